"""No launcher writes past the workspace its size query asks for.  Every workspace is cut by one layout function (csrc/workspace.h)
that also answers the query; here ops._workspace is replaced by one that allocates nbytes + 256 bytes of 0xA5, hands the library
the first nbytes and remembers the buffer.  Every op with a workspace then runs once through its normal Python entry -- the
persistent buffers (dedup plan, block workspace, stream-K hand-over slots, the sharded coreset's rounds) are built inside the
patched scope -- and the last 256 bytes of every buffer must still be 0xA5: an overrun lands in the slack, not in someone else's
memory.  Shapes: the smallest at which every piece of a layout is non-empty and at least two blocks of each kernel run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cmdiad_amd import coreset, ocsvm, ops, runtime  # noqa: E402

DEV = "cuda"
SLACK = 256


@pytest.fixture
def guarded(monkeypatch):
    taken = []

    def workspace(query_name, device, *args):
        nbytes = int(getattr(ops.nat.lib(), query_name)(*args))
        buf = torch.full((nbytes + SLACK,), 0xA5, dtype=torch.uint8, device=device)
        taken.append((query_name, args, buf))
        return buf[:nbytes], nbytes

    monkeypatch.setattr(ops, "_workspace", workspace)
    monkeypatch.setattr(ops, "_streamk_ws", {})       # the per-device stream-K workspace is rebuilt through the guard
    yield taken
    torch.cuda.synchronize()


def _check(taken, queries):
    torch.cuda.synchronize()
    assert {q for q, _, _ in taken} == {"cmdiad_" + q + "_workspace_bytes" for q in queries}, [q for q, _, _ in taken]
    for q, args, buf in taken:
        tail = buf[-SLACK:].cpu().numpy()
        assert (tail == 0xA5).all(), (q, args, np.flatnonzero(tail != 0xA5)[:8])


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_point_cloud_ops_stay_inside_their_workspaces(guarded):
    xyz = _rand(1, 50176, 3, seed=1)                   # just above the register + LDS tiers of the sampling kernel
    ops.fps(xyz, 4)
    cloud = _rand(1, 2048, 3, seed=2)
    ops.knn_group(cloud, cloud[:, :8].contiguous(), 8)
    ops.interp3nn(_rand(1, 300, 3, seed=3), _rand(1, 64, 3, seed=4))
    _check(guarded, ["fps", "knn", "interp3nn"])


def test_coreset_and_ocsvm_stay_inside_their_workspaces(guarded):
    z = _rand(70, 32, seed=5)
    picks16 = coreset.greedy_coreset(z, 8, "FP16")
    coreset.greedy_coreset(z, 8, "TF32")
    bounds = [coreset.shard_rows(70, r, 2) for r in range(2)]
    ranks = [coreset._HipRounds(z) for _ in range(2)]  # a world of 2 on one device, each rank with its own workspace
    keys = torch.zeros((7,), dtype=torch.int64, device=DEV)
    for r in range(7):
        best = torch.zeros((1,), dtype=torch.int64, device=DEV)
        for w in range(2):
            mine = torch.zeros((1,), dtype=torch.int64, device=DEV)
            ranks[w].round(bounds[w][0], bounds[w][1], keys[r - 1:r] if r else None, mine)
            best = torch.maximum(best, mine)
        keys[r] = best[0]
    assert torch.equal(ranks[0].decode(keys, 8), picks16)
    ocsvm.DeviceSGDOneClassSVM(nu=0.5, max_iter=2, random_state=0).fit(_rand(70, 2, seed=6))
    _check(guarded, ["coreset", "coreset_f32", "ocsvm_fit"])
    assert len(guarded) == 5


def test_search_ops_stay_inside_their_workspaces(guarded):
    Q = 1024 + 5                                       # kPlanThreads + 5: two blocks of the plan kernels
    q = _rand(Q, 64, seed=7)
    q[5::100] = q[3]                                   # a few repeated rows
    q16 = q.half()
    plan = ops.rows_dedup_plan(q16, (q16.float() ** 2).sum(1))
    assert 0 < int(plan.count) <= Q
    bank0, bank1, probes = _rand(300, 128, seed=8), _rand(100, 128, seed=9), _rand(4, 128, seed=10)
    ops.reweight_scan(probes, bank0)
    ops.reweight_scan_pair(probes, bank0, ops.bank_block16(bank0), probes, bank1, ops.bank_block16(bank1))
    _check(guarded, ["rows_dedup", "reweight", "reweight_pair"])


def test_transformer_block_and_streamk_stay_inside_their_workspaces(guarded, monkeypatch):
    B, T, C, H, hidden = 1, 65, 128, 2, 512
    g = torch.Generator().manual_seed(11)
    sd = {"norm1.weight": torch.ones(C), "norm1.bias": torch.zeros(C), "norm2.weight": torch.ones(C), "norm2.bias": torch.zeros(C),
          "attn.qkv.weight": torch.randn(3 * C, C, generator=g) / C ** 0.5, "attn.qkv.bias": torch.zeros(3 * C),
          "attn.proj.weight": torch.randn(C, C, generator=g) / C ** 0.5, "attn.proj.bias": torch.zeros(C),
          "mlp.fc1.weight": torch.randn(hidden, C, generator=g) / C ** 0.5, "mlp.fc1.bias": torch.zeros(hidden),
          "mlp.fc2.weight": torch.randn(C, hidden, generator=g) / hidden ** 0.5, "mlp.fc2.bias": torch.zeros(C)}
    x = _rand(B * T, C, seed=12)
    monkeypatch.setenv("CMDIAD_LN_FOLD", "0")
    runtime.transformer_block(x, runtime._pack_block(sd, "", DEV, True), B, T, H, 1e-6, runtime._QkvBuffers())
    monkeypatch.setenv("CMDIAD_LN_FOLD", "1")
    folded, bufs = runtime._pack_block(sd, "", DEV, True), runtime._QkvBuffers()
    assert "qkv_wf" in folded
    runtime.transformer_block(x, folded, B, T, H, 1e-6, bufs, flags=ops.BLOCK_PREP_NEXT)
    runtime.transformer_block(x, folded, B, T, H, 1e-6, bufs, flags=ops.BLOCK_LN1_READY | ops.BLOCK_PREP_NEXT)
    assert torch.isfinite(x).all()
    M, N, K = 256 * 256 + 1, 256, 192                  # 257 tiles of three k-tiles: the smallest eligible product
    assert ops.gemm_streamk_eligible(M, N, K) and not ops.gemm_streamk_eligible(M - 1, N, K) and not ops.gemm_streamk_eligible(M, N, K - 64)
    A, W = _rand(M, K, seed=13).bfloat16(), (_rand(N, K, seed=14) / K ** 0.5).bfloat16()
    bias, res = _rand(N, seed=15), _rand(M, N, seed=16)
    want = ops.gemm(A, W, bias=bias, residual=res, want_f32=True, want_bf16=False)[0]
    assert torch.equal(ops.gemm_streamk(A, W, bias, res), want)
    _check(guarded, ["transformer_block", "gemm_streamk"])
    assert len(guarded) == 3


def test_preprocessing_ops_stay_inside_their_workspaces(guarded):
    pts = _rand(200, 3, seed=17)
    ops.plane_ransac(pts, n=50, iterations=16, distance_threshold=0.5)
    ops.dbscan(0.05 * _rand(500, 3, seed=18), eps=0.02, min_points=5)
    pc = _rand(33, 31, 3, seed=19)
    pc[::3, ::4] = 0.0                                 # invalid pixels
    ops.scan_edges(pc)
    ops.scan_compact(pc)
    _check(guarded, ["plane_ransac", "dbscan", "scan_edges", "scan_compact"])


def test_metrics_ops_stay_inside_their_workspaces(guarded):
    maps = _rand(2, 17, 19, seed=20).double()
    labels, n_comp, comp_offset, comp_size, _ = ops.ccl_label((maps > 0.3).to(torch.uint8))
    count, _, _ = ops.region_table(maps, labels, n_comp, comp_offset, comp_size)
    assert int(count.sum()) > 0
    keys = torch.randint(0, 2 ** 62, (4096 + 7,), generator=torch.Generator().manual_seed(21)).to(DEV)   # kSortTile + 7
    want = torch.sort(keys).values
    assert torch.equal(ops.sort_u64_(keys), want)
    _check(guarded, ["ccl", "region_table", "sort_u64"])
