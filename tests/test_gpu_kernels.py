"""GPU parity tests, kernel by kernel, through the C ABI (cmdiad_amd.ops -> libcmdiad_hip.so) against the
CPU oracle (oracle/) on the same seeded inputs.  Integer/index outputs must be bit-exact; floating
point outputs are compared with the tolerance written next to each assertion."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import need_ab_variants  # noqa: E402
from cmdiad_amd import engine as eng  # noqa: E402

from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd.synth import synth_cloud, synth_cloud_fixed_n  # noqa: E402
from oracle import kernels as ok  # noqa: E402
from oracle import scoring  # noqa: E402

DEV = "cuda"


def _cloud(seed, frac):
    pc, nz = scoring.unorganize_no_zeros(synth_cloud(seed, frac))
    return np.ascontiguousarray(pc[0].T.numpy()), nz  # [N,3]


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------ FPS / kNN
@pytest.fixture(params=["1", "0"], ids=["pk", "reg"])
def fps_variant(request, monkeypatch):
    """Both formulations of the FPS round (fps.hip: packed-math + deferred argmax, and the per-slot (value, slot) one)."""
    if request.param == "0":
        need_ab_variants("fps_reg_kernel")
    monkeypatch.setenv("CMDIAD_FPS_PK", request.param)


@pytest.mark.parametrize("frac,G", [(0.06, 64), (0.2, 256), (0.45, 1024), (0.62, 128)])
def test_fps_bit_exact(frac, G, fps_variant):
    xyz, _ = _cloud(3, frac)  # N ~ 3k / 10k / 22.6k (register path, 512x48) / 31k (memory fallback)
    idx_ref, cen_ref = ok.fps(xyz[None], G)
    idx, cen = ops.fps(torch.from_numpy(xyz[None]).to(DEV), G)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_ref)
    np.testing.assert_array_equal(cen.cpu().numpy(), cen_ref)


def test_fps_batched_ragged_and_skip_rule(fps_variant):
    a, _ = _cloud(4, 0.1)
    b, _ = _cloud(5, 0.07)
    b[17] = 0.001  # |p|^2 <= 1e-3 -> skipped by the sampler (never selected), cmdiad_oracle.c:orc_fps
    N = max(len(a), len(b))
    xyz = np.zeros((2, N, 3), np.float32)
    xyz[0, :len(a)] = a
    xyz[1, :len(b)] = b
    nv = torch.tensor([len(a), len(b)], dtype=torch.int32)
    idx, _ = ops.fps(torch.from_numpy(xyz).to(DEV), 96, n_valid=nv.to(DEV))
    np.testing.assert_array_equal(idx[0].cpu().numpy(), ok.fps(a[None], 96)[0][0])
    ref_b = ok.fps(b[None], 96)[0][0]
    np.testing.assert_array_equal(idx[1].cpu().numpy(), ref_b)
    assert 17 not in ref_b


def test_fps_duplicate_points_tie_rule(fps_variant):
    xyz, _ = _cloud(6, 0.05)
    xyz = np.concatenate([xyz, xyz[:500]], 0)  # exact duplicates -> exact distance ties -> lowest index wins
    idx, _ = ops.fps(torch.from_numpy(xyz[None]).to(DEV), 200)
    np.testing.assert_array_equal(idx.cpu().numpy(), ok.fps(xyz[None], 200)[0])


def test_fps_mostly_skipped_and_all_skipped_clouds(fps_variant):
    """Whole waves of skipped points (|p|^2 <= 1e-3), more samples than valid points (running minima reach 0: ties at 0
    resolve to the lowest index), and a cloud with no valid point at all (every pick is index 0)."""
    rs = np.random.RandomState(3)
    xyz = (rs.rand(3000, 3).astype(np.float32) - 0.5) * 0.02  # all inside the skip radius
    xyz[2000:2040] = rs.rand(40, 3).astype(np.float32) + 0.5   # 40 valid points in the middle
    idx, cen = ops.fps(torch.from_numpy(xyz[None]).to(DEV), 64)
    ref_idx, ref_cen = ok.fps(xyz[None], 64)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(cen.cpu().numpy(), ref_cen)
    xyz[2000:2040] *= 0.001
    idx, _ = ops.fps(torch.from_numpy(xyz[None]).to(DEV), 16)
    np.testing.assert_array_equal(idx.cpu().numpy(), ok.fps(xyz[None], 16)[0])
    assert (idx == 0).all()


def _dense_cloud(n, seed):
    """n distinct points of a bumpy sheet (as the organised clouds: |p|^2 ~ 0.25, far outside the skip radius)."""
    rs = np.random.RandomState(seed)
    xy = (rs.rand(n, 2).astype(np.float32) - 0.5) * 0.2
    z = (0.5 + 0.03 * np.sin(25 * xy[:, 0]) * np.cos(31 * xy[:, 1]) + 1e-4 * rs.randn(n)).astype(np.float32)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32)


def test_fps_ragged_batch_every_cloud_takes_its_own_path():
    """csrc/fps.hip fps_ragged_kernel: per-cloud dispatch on n_valid (not on the padded batch maximum).  One batch holds clouds
    for every branch -- 40 / 48 / 56 points per lane in registers (with the bucket boundaries), registers + the LDS tier (28 673
    ... 38 400 points), registers + LDS + the global tier (above) -- and each must equal the oracle's FPS of that cloud alone;
    bench.py's `var_n` shape (one 30 k-point cloud among 24 k-point clouds) is the second batch."""
    for sizes, G in (((17000, 20480, 20481, 24576, 28672, 28673, 32614, 38400, 38401, 44000), 160),
                     ((24576, 24576, 30011, 24576), 1024)):
        N = (max(sizes) + 255) // 256 * 256
        xyz = np.zeros((len(sizes), N, 3), np.float32)
        clouds = []
        for i, n in enumerate(sizes):
            c = _dense_cloud(n, 40 + i)
            c[n // 2] = 0.001                     # one skipped point per cloud (|p|^2 <= 1e-3)
            if n > 28672:
                c[n - 5] = c[3]                   # an exact duplicate in the TAIL tiers of a register point: ties -> lowest index
            clouds.append(c)
            xyz[i, :n] = c
        nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
        idx, cen = ops.fps(torch.from_numpy(xyz).to(DEV), G, n_valid=nv)
        for i, c in enumerate(clouds):
            ref_idx, ref_cen = ok.fps(c[None], G)
            np.testing.assert_array_equal(idx[i].cpu().numpy(), ref_idx[0], err_msg=f"cloud of {sizes[i]} points")
            np.testing.assert_array_equal(cen[i].cpu().numpy(), ref_cen[0])


def test_fps_tail_tiers_hold_the_farthest_points():
    """A cloud whose farthest points all lie beyond the register tier (indices >= 28 672): most winners then come from the LDS
    and global tiers, including exact ties between tail points (lowest index wins) and with register points."""
    n = 41000
    c = _dense_cloud(n, 77)
    c[:28672, :2] *= 0.05                         # the register tier is a small patch in the middle, the rest surrounds it
    c[40000:40200] = c[30000:30200]               # exact duplicates inside the tail: LDS tier vs global tier
    idx, cen = ops.fps(torch.from_numpy(c[None]).to(DEV), 300)
    ref_idx, ref_cen = ok.fps(c[None], 300)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(cen.cpu().numpy(), ref_cen)
    assert (ref_idx >= 28672).mean() > 0.5 and (ref_idx >= 38400).any()


@pytest.fixture(params=["1", "0"], ids=["wave", "block"])
def knn_variant(request, monkeypatch):
    """Both formulations of the kNN grouping (knn_group.hip: a wave owns its centres with an in-register sorting network, and
    the block-wide LDS bitonic sort)."""
    if request.param == "0":
        need_ab_variants("knn_group_kernel")
    monkeypatch.setenv("CMDIAD_KNN_WAVE", request.param)


@pytest.mark.parametrize("frac,G,K", [(0.06, 64, 32), (0.3, 128, 128), (0.1, 70, 100), (0.45, 1024, 128), (0.05, 5, 1), (0.05, 33, 64), (0.05, 16, 65)])
def test_knn_group_bit_exact(frac, G, K, knn_variant):
    xyz, _ = _cloud(7, frac)
    _, cen = ok.fps(xyz[None], G)
    idx_ref, nb_ref = ok.knn_group(xyz[None], cen, K)
    idx, nb = ops.knn_group(torch.from_numpy(xyz[None]).to(DEV), torch.from_numpy(cen).to(DEV), K)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_ref)
    np.testing.assert_array_equal(nb.cpu().numpy(), nb_ref)


def _knn_geometries():
    rs = np.random.RandomState(4)
    sheet = _cloud(31, 0.45)[0]                                                     # a depth-camera sheet (the production case)
    wall = sheet[:, [0, 2, 1]].copy()                                               # the same sheet standing up: grid axes x and z
    blob = rs.rand(6000, 3).astype(np.float32)                                      # a filled cube: the 2-D grid's worst case
    two = np.concatenate([rs.randn(2500, 3) * 0.01, rs.randn(2500, 3) * 0.01 + 5.0]).astype(np.float32)   # two far clusters: empty cells between
    line = np.stack([np.linspace(0, 1, 4000), np.zeros(4000), np.zeros(4000)], 1).astype(np.float32)       # one axis only (second extent 0)
    same = np.tile(np.array([[0.3, -0.2, 0.9]], np.float32), (2100, 1))             # every point identical: h = 0, ties by index
    dup = np.concatenate([sheet[:3000], sheet[:3000]])                              # every point twice
    return dict(sheet=sheet, wall=wall, blob=blob, two_clusters=two, line=line, identical=same, duplicates=dup)


@pytest.mark.parametrize("name", ["sheet", "wall", "blob", "two_clusters", "line", "identical", "duplicates"])
def test_knn_neighbourhood_search_is_the_streaming_search(name, monkeypatch):
    """cmdiad_knn_group_ws (round 6: the cloud binned into a 64 x 64 grid on its two widest axes, a wave scanning the rings of
    cells around its centre until the K-th distance is certified) returns the streaming kernel's and the oracle's neighbours bit
    for bit -- on geometries chosen against it: a standing sheet, a filled cube, two far clusters with empty cells between, points
    on a line, all points identical (a degenerate grid), every point duplicated (ties by index), centres outside the cloud's
    bounding box, K = 1 / 37 / 128, ragged n_valid."""
    pts = _knn_geometries()[name]
    rs = np.random.RandomState(5)
    G = 96
    cen = pts[rs.randint(0, len(pts), G)].copy()
    cen[::7] += rs.randn(len(cen[::7]), 3).astype(np.float32) * 0.05               # off-surface centres
    cen[::13] = pts.min(0) - 0.3                                                    # outside the bounding box
    cen[5::13] = pts.max(0) + 2.0
    N = len(pts) + 300
    xyz = np.zeros((2, N, 3), np.float32)
    xyz[0, :len(pts)] = pts
    n1 = max(2048, len(pts) - 777) if len(pts) > 2900 else len(pts)
    xyz[1, :n1] = pts[:n1]
    xyz[:, len(pts):] = 1e6                                                         # garbage beyond n_valid must not be read as points
    nv = torch.tensor([len(pts), n1], dtype=torch.int32, device=DEV)
    x, c = torch.from_numpy(xyz).to(DEV), torch.from_numpy(np.stack([cen, cen])).to(DEV)
    for K in (1, 37, 128):
        monkeypatch.setenv("CMDIAD_KNN_GRID", "1")
        idx, nb = ops.knn_group(x, c, K, n_valid=nv)
        monkeypatch.setenv("CMDIAD_KNN_GRID", "0")
        idx_s, nb_s = ops.knn_group(x, c, K, n_valid=nv)
        assert torch.equal(idx, idx_s) and torch.equal(nb, nb_s), (name, K)
        for i, n in enumerate((len(pts), n1)):
            ir, nr = ok.knn_group(pts[None, :n], cen[None], K)
            np.testing.assert_array_equal(idx[i].cpu().numpy(), ir[0], err_msg=f"{name} K={K} cloud {i}")
            np.testing.assert_array_equal(nb[i].cpu().numpy(), nr[0], err_msg=f"{name} K={K} cloud {i}")


@pytest.mark.parametrize("name", ["sheet", "wall", "blob", "two_clusters", "line", "identical", "duplicates"])
@pytest.mark.parametrize("scale", [1.0, 700.0], ids=["metres", "large_coordinates"])
def test_interp3nn_neighbourhood_search_is_the_full_search(name, scale, monkeypatch):
    """cmdiad_interp3nn_ws (round 6: the centres binned into a 16 x 16 grid, a point scanning the rings of cells around it until its
    three best values of the reference's distance FORMULA are certified, rounding bound included) returns the full search's and
    the oracle's idx3 / w3 bit for bit -- on the geometries of the kNN test, with centres that are cloud points, off-surface
    points, duplicates of each other (ties by index) and far outliers; and with coordinates x 700 (millimetre-sized numbers: the
    formula -2 a.b + |a|^2 + |b|^2 then carries rounding noise of the order of the centre spacing -- the search must fall back to
    wider rings instead of certifying early)."""
    pts = (_knn_geometries()[name] * scale + (0.0 if scale == 1.0 else 250.0)).astype(np.float32)
    rs = np.random.RandomState(6)
    S = 300
    cen = pts[rs.randint(0, len(pts), S)].copy()
    cen[::9] += (rs.randn(len(cen[::9]), 3) * 0.03 * scale).astype(np.float32)
    cen[7] = cen[3]; cen[250] = cen[3]                                              # identical centres: ties by index
    cen[11] = pts.max(0) + 5.0 * scale                                              # a far outlier stretches the grid
    n = min(len(pts), 6000)
    N = n + 100
    xyz = np.zeros((2, N, 3), np.float32)
    xyz[0, :n] = pts[:n]
    xyz[1, :n - 500] = pts[500:n]
    nv = torch.tensor([n, n - 500], dtype=torch.int32, device=DEV)
    x, c = torch.from_numpy(xyz).to(DEV), torch.from_numpy(np.stack([cen, cen[::-1].copy()])).to(DEV)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "1")
    idx3, w3 = ops.interp3nn(x, c, n_valid=nv)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "0")
    idx_f, w_f = ops.interp3nn(x, c, n_valid=nv)
    assert torch.equal(idx3, idx_f) and torch.equal(w3, w_f), name
    feat = np.zeros((S, 4), np.float32)
    for i, (m, cc) in enumerate(((n, cen), (n - 500, cen[::-1].copy()))):
        _, ir, wr = ok.interp3nn(xyz[i, :m], cc, feat)
        np.testing.assert_array_equal(idx3[i, :m].cpu().numpy(), ir, err_msg=f"{name} cloud {i}")
        np.testing.assert_array_equal(w3[i, :m].cpu().numpy(), wr, err_msg=f"{name} cloud {i}")


def test_interp3nn_far_from_the_origin_falls_back_to_the_whole_grid(monkeypatch):
    """A unit sheet 3 000 units from the origin: the rounding of -2 a.b + |a|^2 + |b|^2 (~2) dwarfs the squared centre spacing, the
    reference's own selection is rounding noise -- the neighbourhood search may not certify on geometry, widens to every centre and
    returns the full search's / the oracle's idx3 and w3 bit for bit (tests/test_neighbourhood_model_cpu.py models the same case)."""
    pts = (_knn_geometries()["sheet"][:5000] + 3000.0).astype(np.float32)
    rs = np.random.RandomState(13)
    cen = pts[rs.randint(0, len(pts), 256)].copy()
    x, c = torch.from_numpy(pts[None]).to(DEV), torch.from_numpy(cen[None]).to(DEV)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "1")
    idx3, w3 = ops.interp3nn(x, c)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "0")
    idx_f, w_f = ops.interp3nn(x, c)
    assert torch.equal(idx3, idx_f) and torch.equal(w3, w_f)
    _, ir, wr = ok.interp3nn(pts, cen, np.zeros((256, 4), np.float32))
    np.testing.assert_array_equal(idx3[0].cpu().numpy(), ir)
    np.testing.assert_array_equal(w3[0].cpu().numpy(), wr)


@pytest.mark.parametrize("K", [1, 128])
def test_knn_neighbourhood_search_at_its_smallest_cloud(K, monkeypatch):
    """The edges of the kNN grid path (csrc/cell_grid.h builder under knn_grid_build_kernel): N = 2 048, the smallest size that
    takes the grid, so the 1 024-thread builder has two points per thread at most; clouds of 128 / 129 / 2 047 / 2 048 valid
    points with garbage behind them (whole waves of the builder idle, K = 128 = every point of the first cloud); G = 5, so the
    last query block has idle waves.  Grid == streaming == oracle per cloud, indices and neighbourhoods."""
    N, G, sizes = 2048, 5, (128, 129, 2047, 2048)
    rs = np.random.RandomState(21)
    xyz = np.full((len(sizes), N, 3), 1e6, np.float32)                              # garbage beyond n_valid must not be read as points
    cen = np.zeros((len(sizes), G, 3), np.float32)
    for i, n in enumerate(sizes):
        xyz[i, :n] = _dense_cloud(n, 60 + i)
        cen[i] = xyz[i, rs.randint(0, n, G)]
    cen[:, 4] += 0.01                                                               # one centre off the surface
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    x, c = torch.from_numpy(xyz).to(DEV), torch.from_numpy(cen).to(DEV)
    monkeypatch.setenv("CMDIAD_KNN_GRID", "1")
    idx, nb = ops.knn_group(x, c, K, n_valid=nv)
    monkeypatch.setenv("CMDIAD_KNN_GRID", "0")
    idx_s, nb_s = ops.knn_group(x, c, K, n_valid=nv)
    assert torch.equal(idx, idx_s) and torch.equal(nb, nb_s)
    for i, n in enumerate(sizes):
        ir, nr = ok.knn_group(xyz[i:i + 1, :n], cen[i:i + 1], K)
        np.testing.assert_array_equal(idx[i].cpu().numpy(), ir[0], err_msg=f"cloud of {n} points")
        np.testing.assert_array_equal(nb[i].cpu().numpy(), nr[0], err_msg=f"cloud of {n} points")


@pytest.mark.parametrize("S", [64, 65, 1024, 4096])
def test_interp3nn_neighbourhood_search_at_the_edges_of_the_centre_count(S, monkeypatch):
    """The edges of the 3-NN grid path (csrc/cell_grid.h builder under interp3nn_bin_kernel): S = 64, the fewest centres that take
    the grid (a quarter of the builder's threads own one), 65, the production 1 024 and 4 096, the most the entry accepts -- its
    83 KB of LDS need the launch attribute raised (launch_lds); N = 257 (a second block with one point), a second cloud with ONE
    valid point.  Centres are cloud points, two identical (ties by index), one far outlier.  Grid == full == oracle."""
    N, sizes = 257, (257, 1)
    rs = np.random.RandomState(22)
    pts = _dense_cloud(N, 70)
    cen = pts[rs.randint(0, N, S)].copy()
    cen[1::2] += (rs.randn(len(cen[1::2]), 3) * 0.003).astype(np.float32)
    cen[7] = cen[3]                                                                 # identical centres: ties by index
    cen[11] = pts.max(0) + 5.0                                                      # a far outlier stretches the grid
    cens = np.stack([cen, cen[::-1].copy()])
    xyz = np.stack([pts, pts[::-1].copy()])
    nv = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    x, c = torch.from_numpy(xyz).to(DEV), torch.from_numpy(cens).to(DEV)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "1")
    idx3, w3 = ops.interp3nn(x, c, n_valid=nv)
    monkeypatch.setenv("CMDIAD_INTERP_GRID", "0")
    idx_f, w_f = ops.interp3nn(x, c, n_valid=nv)
    assert torch.equal(idx3, idx_f) and torch.equal(w3, w_f)
    feat = np.zeros((S, 4), np.float32)
    for i, m in enumerate(sizes):
        _, ir, wr = ok.interp3nn(xyz[i, :m], cens[i], feat)
        np.testing.assert_array_equal(idx3[i, :m].cpu().numpy(), ir, err_msg=f"cloud {i}")
        np.testing.assert_array_equal(w3[i, :m].cpu().numpy(), wr, err_msg=f"cloud {i}")


def test_knn_group_production_instantiation_ragged():
    """The grid the pipeline runs (knn_wave_kernel<4, 4>: four waves per block, four centres per wave, chosen when
    B * ceil(G / 16) >= 512) on eight ragged clouds, bit for bit against the oracle and identical over repeated launches.  The
    smaller cases above all select the one-centre-per-wave instantiation: a round-4 form of the per-centre loop (lane masks of
    all four centres taken before the first centre's work) returned wrong neighbours for the SECOND centre of every wave, on this
    instantiation only, and no test saw it -- bench.py's step-to-step comparison did."""
    B, G, K = 8, 1024, 128
    clouds = [_cloud(20 + i, 0.05 + 0.01 * i)[0] for i in range(B)]
    N = max(len(c) for c in clouds)
    xyz = np.zeros((B, N, 3), np.float32)
    for i, c in enumerate(clouds):
        xyz[i, :len(c)] = c
    nv = torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=DEV)
    cen = np.stack([ok.fps(c[None], G)[1][0] for c in clouds])
    ref = [ok.knn_group(c[None], cen[i:i + 1], K) for i, c in enumerate(clouds)]
    x, c = torch.from_numpy(xyz).to(DEV), torch.from_numpy(cen).to(DEV)
    first = None
    for rep in range(3):
        idx, nb = ops.knn_group(x, c, K, n_valid=nv)
        for i in range(B):
            np.testing.assert_array_equal(idx[i].cpu().numpy(), ref[i][0][0], err_msg=f"cloud {i}, launch {rep}")
            np.testing.assert_array_equal(nb[i].cpu().numpy(), ref[i][1][0], err_msg=f"cloud {i}, launch {rep}")
        first = idx if first is None else first
        assert torch.equal(idx, first)


def test_knn_group_ties_and_ragged(knn_variant):
    a, _ = _cloud(8, 0.08)
    a = np.concatenate([a, a[:300]], 0)  # duplicates: ties at equal d2 resolved by index
    b, _ = _cloud(9, 0.05)
    N = max(len(a), len(b))
    xyz = np.zeros((2, N, 3), np.float32)
    xyz[0, :len(a)] = a
    xyz[1, :len(b)] = b
    nv = torch.tensor([len(a), len(b)], dtype=torch.int32, device=DEV)
    cen = np.stack([ok.fps(a[None], 50)[1][0], ok.fps(b[None], 50)[1][0]])  # G=50: not a multiple of 4
    idx, nb = ops.knn_group(torch.from_numpy(xyz).to(DEV), torch.from_numpy(cen).to(DEV), 64, n_valid=nv)
    for i, cl in enumerate((a, b)):
        ir, nr = ok.knn_group(cl[None], cen[i:i + 1], 64)
        np.testing.assert_array_equal(idx[i].cpu().numpy(), ir[0])
        np.testing.assert_array_equal(nb[i].cpu().numpy(), nr[0])


# ------------------------------------------------------------------------------------------ unorganize / interp / pool
def test_unorganize_matches_reference_semantics():
    pcs = torch.cat([synth_cloud(11, 0.4), synth_cloud(12, 0.55), synth_cloud_fixed_n(13, 24576)], 0)
    xyz, nz, pix2pt, nv = ops.unorganize(pcs.to(DEV))
    for b in range(3):
        pc, nzr = scoring.unorganize_no_zeros(pcs[b:b + 1])
        n = pc.shape[2]
        assert int(nv[b]) == n
        np.testing.assert_array_equal(nz[b, :n].cpu().numpy(), nzr)
        np.testing.assert_array_equal(xyz[b, :n].cpu().numpy(), pc[0].T.numpy())
        p2p = pix2pt[b].cpu().numpy()
        assert (p2p >= 0).sum() == n and np.array_equal(p2p[nzr], np.arange(n))
    assert int(nv[2]) == 24576


def test_interp3nn_indices_bit_exact_and_patch_fused():
    organized = synth_cloud(14, 0.3)
    pc, nzr = scoring.unorganize_no_zeros(organized)
    xyz = np.ascontiguousarray(pc[0].T.numpy())
    N, S, D = len(xyz), 256, 64
    _, cen = ok.fps(xyz[None], S)
    feat = torch.randn(S, D, generator=torch.Generator().manual_seed(15)).numpy()
    out_ref, idx_ref, w_ref = ok.interp3nn(xyz, cen[0], feat)
    dxyz, dnz, pix2pt, nv = ops.unorganize(organized.to(DEV))
    idx3, w3 = ops.interp3nn(dxyz, torch.from_numpy(cen).to(DEV), n_valid=nv)
    np.testing.assert_array_equal(idx3[0, :N].cpu().numpy(), idx_ref)
    np.testing.assert_array_equal(w3[0, :N].cpu().numpy(), w_ref)  # same op order, IEEE division
    dfeat = torch.from_numpy(feat[None]).to(DEV)
    g = ops.interp_gather(dfeat, idx3, w3, n_valid=nv)
    np.testing.assert_array_equal(g[0, :N].cpu().numpy(), out_ref)
    for P in (56, 28):
        ref = ok.xyz_patch(out_ref, nzr, 224, P)
        p32, p16 = ops.xyz_patch_fused(dfeat, idx3, w3, pix2pt, 224, P, want_bf16=True)
        # same linear map, different summation order: fp32 round-off only
        np.testing.assert_allclose(p32[0].cpu().numpy(), ref, rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(p16[0].float().cpu().numpy(), ref, rtol=1e-2, atol=1e-3)
    # fused normalisation (multiple_features.py:976)
    p32n, _ = ops.xyz_patch_fused(dfeat, idx3, w3, pix2pt, 224, 56, mean=0.25, inv_std=1 / 1.7)
    np.testing.assert_allclose(p32n[0].cpu().numpy(), (ok.xyz_patch(out_ref, nzr, 224, 56) - 0.25) / 1.7, rtol=2e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------ GEMM family
@pytest.mark.parametrize("M,N,K,panel_min,wide", [(128, 128, 64, None, None), (300, 384, 192, None, None), (785, 768, 768, None, None),
                                                   (1000, 1920, 768, None, None), (300, 384, 192, "1", None), (1000, 1156, 512, "1", None),
                                                   (300, 384, 192, None, "8"), (1000, 1156, 512, None, "4"), (785, 768, 768, None, "8"),
                                                   (600, 640, 1024, None, "4")])
def test_gemm_epilogues(M, N, K, panel_min, wide, monkeypatch):
    if panel_min:  # panel mode: one block walks up to 8 N tiles (K <= 512 products)
        monkeypatch.setenv("CMDIAD_GEMM_PANEL_MIN", panel_min)
    if wide:  # the 4-wave 256-row shapes (gemm_wide.h): 8 = 256x256, 4 = 256x128; ragged M and N tiles included
        need_ab_variants("gemm_std_wide_kernel")
        monkeypatch.setenv("CMDIAD_GEMM_WIDE", wide)
    g = torch.Generator().manual_seed(M + N + K)
    A = _bf(torch.randn(M, K, generator=g))
    W = _bf(torch.randn(N, K, generator=g) / K ** 0.5)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    gb = torch.randn((M + 31) // 32, N, generator=g)
    ref = A.double() @ W.double().T
    dA, dW = A.to(DEV).bfloat16(), W.to(DEV).bfloat16()
    o32, o16 = ops.gemm(dA, dW, want_f32=True)
    np.testing.assert_allclose(o32.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)  # fp32 accumulate order
    np.testing.assert_allclose(o16.float().cpu().numpy(), ref.numpy(), rtol=8e-3, atol=8e-3)  # bf16 rounding 2^-8
    o32, _ = ops.gemm(dA, dW, bias=bias.to(DEV), act=ops.ACT_GELU, residual=res.to(DEV), want_f32=True, want_bf16=False)
    want = torch.nn.functional.gelu(ref + bias.double()) + res.double()
    np.testing.assert_allclose(o32.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
    o32, _ = ops.gemm(dA, dW, bias=bias.to(DEV), act=ops.ACT_RELU, group_bias=gb.to(DEV), group_rows=32,
                      want_f32=True, want_bf16=False)
    want = torch.relu(ref + bias.double() + gb.double().repeat_interleave(32, 0)[:M])
    np.testing.assert_allclose(o32.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
    # in-place residual stream (out aliases residual), as the transformer blocks use it
    x = res.clone().to(DEV)
    ops.gemm(dA, dW, bias=bias.to(DEV), residual=x, out_f32=x, want_bf16=False)
    np.testing.assert_allclose(x.cpu().numpy(), (ref + bias.double() + res.double()).numpy(), rtol=1e-4, atol=1e-4)


def test_gemm_persistent_256_tile_matches_128_tile(monkeypatch):
    """cmdiad_gemm_bf16 on the two-group persistent 256 x 256 kernel (gemm_std_pp3_kernel: one block per CU walks a job list;
    production choice for the fc1 products at batch 32) gives bit for bit what the 128 x 128 kernel gives -- same K order,
    same epilogue arithmetic -- on shapes with ragged M, more and fewer jobs than blocks, every epilogue it supports (the
    calls it does not take -- fp32 / residual outputs -- fall through to the 128 x 128 kernel in both modes).  The last shape
    is 603 jobs on 201 blocks at the minimum K of three K-tiles, ragged last M tile: three jobs per block, so a whole job
    lies between two job boundaries of both the stream's and the consumer's copy of the job cursor."""
    g = torch.Generator().manual_seed(77)
    for M, N, K in ((1000, 512, 192), (70000, 256, 192), (3 * 785, 1536, 768), (40000, 512, 256), (51217, 768, 192)):
        A = _bf(torch.randn(M, K, generator=g))
        W = _bf(torch.randn(N, K, generator=g) / K ** 0.5)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        dA, dW = A.to(DEV).bfloat16(), W.to(DEV).bfloat16()
        got = {}
        for mode in ("0", "pp3"):
            monkeypatch.setenv("CMDIAD_GEMM_PP3", "1" if mode == "pp3" else "0")   # two-group persistent kernel (gemm_pp3.h)
            o32, o16 = ops.gemm(dA, dW, bias=bias.to(DEV), act=ops.ACT_GELU, want_f32=True, want_bf16=True)
            _, g16 = ops.gemm(dA, dW, bias=bias.to(DEV), act=ops.ACT_GELU)     # bf16-only output: the form the pp3 kernel takes
            x = res.clone().to(DEV)
            ops.gemm(dA, dW, bias=bias.to(DEV), residual=x, out_f32=x, want_bf16=False)
            _, r16 = ops.gemm(dA, dW, bias=bias.to(DEV), act=ops.ACT_RELU)
            _, n16 = ops.gemm(dA, dW, bias=bias.to(DEV))
            got[mode] = (o32.clone(), o16.clone(), x, r16.clone(), g16.clone(), n16.clone())
        for a, b in zip(got["0"], got["pp3"]):
            assert torch.equal(a, b)
        assert torch.equal(got["0"][1], got["0"][4])
        ref = A.double() @ W.double().T
        want = torch.nn.functional.gelu(ref + bias.double())
        np.testing.assert_allclose(got["pp3"][0].cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got["pp3"][4].float().cpu().numpy(), want.numpy(), rtol=8e-3, atol=8e-3)   # the bf16 form pp3 takes
        np.testing.assert_allclose(got["pp3"][2].cpu().numpy(), (ref + bias.double() + res.double()).numpy(), rtol=1e-4, atol=1e-4)


def test_gemm_streamk_matches_128_tile_bit_for_bit():
    """cmdiad_gemm_streamk_bf16 (csrc/gemm_sk.hip: the (tile, k-tile) list of the N = 768 residual products cut into one range
    per CU, tiles shared by two blocks finished in order through parked accumulators) against cmdiad_gemm_bf16's 128 x 128
    kernel on ViT-B/8's batch-32 shapes: fc2 (K = 3072), proj (K = 768), ragged and whole last M tile, in place on the residual
    stream -- identical bits, launch after launch on one workspace (the hand-over counters return to zero)."""
    g = torch.Generator().manual_seed(91)
    for M, N, K in ((32 * 785, 768, 3072), (32 * 785, 768, 768), (100 * 256, 768, 1536), (24000, 1024, 1024)):
        assert ops.gemm_streamk_eligible(M, N, K), (M, N, K)
        dA = (torch.randn(M, K, generator=g)).to(DEV).bfloat16()
        dW = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).bfloat16()
        bias, res = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
        want = res.clone()
        ops.gemm(dA, dW, bias=bias, residual=want, out_f32=want, want_bf16=False)
        for rep in range(3):
            x = res.clone()
            ops.gemm_streamk(dA, dW, bias, x, out_f32=x)                    # in place, as the transformer block runs it
            assert torch.equal(x, want), (M, N, K, rep, float((x - want).abs().max()))
        out = ops.gemm_streamk(dA, dW, bias, res)                           # separate output buffer
        assert torch.equal(out, want)
        ref = dA[:512].double() @ dW.double().T + bias.double() + res[:512].double()
        np.testing.assert_allclose(want[:512].cpu().double().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=1e-4)
    for M, N, K in ((2 * 785, 768, 3072), (32 * 785, 384, 1536), (32 * 785, 3072, 768), (70000, 768, 768)):
        assert not ops.gemm_streamk_eligible(M, N, K)                       # too few tiles / N % 256 / two or more tiles per CU


def test_gemm_residual_on_wide_tiles_matches_128_tile_bit_for_bit(monkeypatch):
    """CMDIAD_GEMM_RES_WIDE=1 (a measurement switch, profiles/r4_notes.md section 12): the in-place residual products of
    cmdiad_gemm_bf16 on the two-group 256 x 256 kernel with one whole tile per block -- identical bits to the 128 x 128 kernel,
    ragged last M tile included; shapes it is not legal for (N % 256) fall through to the default kernel."""
    g = torch.Generator().manual_seed(92)
    for M, N, K in ((32 * 785, 768, 768), (9 * 256 + 17, 512, 1536), (300, 256, 192), (4000, 384, 384)):
        dA = (torch.randn(M, K, generator=g)).to(DEV).bfloat16()
        dW = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).bfloat16()
        bias, res = torch.randn(N, generator=g).to(DEV), torch.randn(M, N, generator=g).to(DEV)
        monkeypatch.setenv("CMDIAD_GEMM_RES_WIDE", "0")
        want = res.clone()
        ops.gemm(dA, dW, bias=bias, residual=want, out_f32=want, want_bf16=False)
        monkeypatch.setenv("CMDIAD_GEMM_RES_WIDE", "1")
        x = res.clone()
        ops.gemm(dA, dW, bias=bias, residual=x, out_f32=x, want_bf16=False)
        assert torch.equal(x, want), (M, N, K, float((x - want).abs().max()))
        out, _ = ops.gemm(dA, dW, bias=bias, residual=res, want_f32=True, want_bf16=False)   # separate output buffer
        assert torch.equal(out, want)


def test_gemm_identity_asymmetric_layout():
    # A = I against an asymmetric W catches any row/column swap in the accumulator mapping
    K = 128
    A = torch.eye(K)
    W = torch.arange(K * K, dtype=torch.float32).reshape(K, K) % 251 - 125.0
    o32, _ = ops.gemm(A.to(DEV).bfloat16(), W.to(DEV).bfloat16(), want_f32=True)
    np.testing.assert_array_equal(o32.cpu().numpy(), W.T.numpy())


@pytest.mark.parametrize("B,T,C", [(2, 785, 768), (1, 1024, 384), (3, 200, 128)])
def test_qkv_and_attention(B, T, C):
    H = C // 64
    Tp = (T + 63) // 64 * 64
    g = torch.Generator().manual_seed(B * T + C)
    x = _bf(torch.randn(B * T, C, generator=g))
    W = _bf(torch.randn(3 * C, C, generator=g) / C ** 0.5)
    bias = 0.1 * torch.randn(3 * C, generator=g)
    q = torch.zeros(B, H, Tp, 64, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros_like(q)
    vt = torch.zeros(B, H, 64, Tp, dtype=torch.bfloat16, device=DEV)
    ops.gemm_qkv(x.to(DEV).bfloat16(), W.to(DEV).bfloat16(), bias.to(DEV), B, T, q, k, vt)
    qkv = (x.double() @ W.double().T + bias.double()).reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    LOG2E = 1.4426950408889634
    np.testing.assert_allclose(q[:, :, :T].float().cpu().numpy(), (qkv[0] * 0.125 * LOG2E).numpy(), rtol=8e-3, atol=8e-3)
    np.testing.assert_allclose(k[:, :, :T].float().cpu().numpy(), qkv[1].numpy(), rtol=8e-3, atol=8e-3)
    np.testing.assert_allclose(vt[:, :, :, :T].float().cpu().numpy(), qkv[2].transpose(-1, -2).numpy(), rtol=8e-3, atol=8e-3)
    assert float(q[:, :, T:].abs().max() if Tp > T else 0) == 0.0  # padding untouched
    out = ops.attention(q, k, vt, B, H, T)
    # reference from the SAME bf16-rounded q/k/v (isolates the attention kernel): fp64 softmax(q k^T) v
    qd, kd, vd = q[:, :, :T].double().cpu(), k[:, :, :T].double().cpu(), vt[:, :, :, :T].double().cpu().transpose(-1, -2)
    ref = (torch.softmax(qd @ kd.transpose(-1, -2) / LOG2E, -1) @ vd).transpose(1, 2).reshape(B * T, C)
    # P is rounded to bf16 before P.V and the output is bf16: |err| <~ 2^-8 * |v|_max-ish
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), rtol=2e-2, atol=2e-2)
    assert float((out.float().cpu() - ref).abs().mean()) < 3e-3


def test_attention_peaked_rows_exercise_rescale():
    # one key per query dominates and sits in a LATE tile: the running max must jump (online-softmax rescale)
    B, H, T = 1, 1, 300
    Tp = 320
    g = torch.Generator().manual_seed(5)
    q = torch.zeros(B, H, Tp, 64)
    k = torch.zeros(B, H, Tp, 64)
    v = torch.zeros(B, H, Tp, 64)
    q[0, 0, :T] = torch.randn(T, 64, generator=g)
    k[0, 0, :T] = torch.randn(T, 64, generator=g)
    v[0, 0, :T] = torch.randn(T, 64, generator=g)
    k[0, 0, 280] = 4.0 * q[0, 0, 10]  # spike for query 10 in the last tile
    q, k, v = _bf(q), _bf(k), _bf(v)
    out = ops.attention(q.to(DEV).bfloat16(), k.to(DEV).bfloat16(), v.transpose(-1, -2).contiguous().to(DEV).bfloat16(), B, H, T)
    # the kernel's contract: q carries log2(e), i.e. it computes softmax_2(q.k) = softmax(q.k * ln 2)
    ref = torch.softmax(q[0, 0, :T].double() @ k[0, 0, :T].double().T * np.log(2.0), -1) @ v[0, 0, :T].double()
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("step", [3.0, 6.0, 7.9, 8.1, 20.0, -6.0])
def test_attention_reference_moves_lazily(step):
    """The softmax reference of a wave moves only when a score exceeds it by more than 8 (log2 units): scores that climb by `step`
    per 64-key tile stay below that for one tile or more (P up to 2^8 against the stale reference), cross it, or fall; one query of
    every wave climbs while the other 31 do not (the decision is wave-uniform, the amount per query).  Against float64 softmax_2."""
    B, H, T = 2, 3, 600
    Tp = 640
    g = torch.Generator().manual_seed(int(abs(step) * 10))
    q = torch.zeros(B, H, Tp, 64)
    k = torch.zeros(B, H, Tp, 64)
    v = torch.zeros(B, H, Tp, 64)
    q[:, :, :T] = 0.3 * torch.randn(B, H, T, 64, generator=g)
    k[:, :, :T] = torch.randn(B, H, T, 64, generator=g)
    v[:, :, :T] = torch.randn(B, H, T, 64, generator=g)
    q[:, :, :T:32, :] = 0.0
    q[:, :, :T:32, 5] = 1.0                                       # query 0 of every wave reads column 5 of the keys only ...
    k[:, :, :T, 5] = step * (torch.arange(T) // 64).float()       # ... which climbs (or falls) by `step` per tile
    q, k, v = _bf(q), _bf(k), _bf(v)
    out = ops.attention(q.to(DEV).bfloat16(), k.to(DEV).bfloat16(), v.transpose(-1, -2).contiguous().to(DEV).bfloat16(), B, H, T)
    sc = q[:, :, :T].double() @ k[:, :, :T].double().transpose(-1, -2)
    ref = (torch.softmax(sc * np.log(2.0), -1) @ v[:, :, :T].double()).transpose(1, 2).reshape(B * T, H * 64)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), rtol=2e-2, atol=2e-2)
    assert float((out.float().cpu() - ref).abs().mean()) < 3e-3


@pytest.mark.parametrize("M,C", [(785, 768), (1024, 384), (5, 128)])
def test_layernorm(M, C):
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, C, generator=g) * 3 + 1
    add = torch.randn(M, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dx = x.clone().to(DEV)
    y = ops.layernorm(dx, gamma.to(DEV), beta.to(DEV), 1e-6)
    ref = torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-6)
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), rtol=8e-3, atol=8e-3)
    o32 = torch.empty(M, 2 * C, device=DEV)
    ops.layernorm(dx, gamma.to(DEV), beta.to(DEV), 1e-5, add=add.to(DEV), out_f32=o32[:, C:], want_bf16=False)
    np.testing.assert_allclose(dx.cpu().numpy(), (x + add).numpy(), rtol=0, atol=0)
    ref = torch.nn.functional.layer_norm(x + add, (C,), gamma, beta, 1e-5)
    np.testing.assert_allclose(o32[:, C:].cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("Mg,panel_min,wide", [(32, None, "0"), (128, None, "0"), (128, "1", "0"), (32, "1", "0"),
                                                (128, None, "8"), (32, None, "4"), (64, None, "4"), (128, None, "4")])
def test_pointmae_encoder_stages(Mg, panel_min, wide, monkeypatch):
    from oracle import nets
    if panel_min:  # one block walks every N tile of its M panel
        monkeypatch.setenv("CMDIAD_GEMM_PANEL_MIN", panel_min)
    monkeypatch.setenv("CMDIAD_GEMM_WIDE", wide)  # "0": 128x128 shape; "4"/"8": the 256-row shapes production picks at 4.2 M rows
    sd = nets.synth_state_dict("pointmae", 21)
    groups = 24
    g = torch.Generator().manual_seed(Mg)
    nb = 0.02 * torch.randn(1, groups, Mg, 3, generator=g)
    from cmdiad_amd.runtime import fold_pointmae_encoder
    w = fold_pointmae_encoder(sd, "encoder.", DEV)
    h2, g32, g16 = ops.encoder_stage1(nb.reshape(-1, 3).contiguous().to(DEV), w["w1b1"], w["W2"], w["b2"], groups, Mg)
    gb, _ = ops.gemm(g16, w["W3a"], bias=w["b3"], want_f32=True, want_bf16=False)
    _, h3 = ops.gemm(h2, w["W3b"], act=ops.ACT_RELU, group_bias=gb, group_rows=Mg)
    tok, _ = ops.gemm_groupmax(h3, w["W4"], w["b4"], groups, Mg)
    with torch.no_grad():
        ref = nets.pointmae_encoder(sd, nb)[0]
    # three chained bf16 GEMMs against the fp32 oracle: relative error ~ 3 * 2^-8 of the token scale
    scale = ref.abs().mean().item()
    err = (tok.cpu() - ref).abs()
    assert err.mean().item() < 0.01 * scale and err.max().item() < 0.08 * scale, (err.mean().item(), err.max().item(), scale)


@pytest.mark.parametrize("groups,Mg", [(24, 128), (300, 128), (700, 128), (1028, 32), (1030, 32), (514, 64), (7, 32), (9, 64)])
def test_encoder_stage1_against_direct_reference(groups, Mg):
    """cmdiad_encoder_stage1 (models/models.py:188-195: conv1 + BN + ReLU, conv2, per-group max) against the same arithmetic in
    torch: persistent kernel when groups * Mg is a multiple of 128 (1, 2 and 3 tiles per block: the coordinate prefetch runs two
    tiles ahead), the once-per-block kernel for ragged row counts."""
    from oracle import nets
    from cmdiad_amd.runtime import fold_pointmae_encoder
    w = fold_pointmae_encoder(nets.synth_state_dict("pointmae", 21), "encoder.", DEV)
    g = torch.Generator().manual_seed(groups * 1000 + Mg)
    nb = (0.05 * torch.randn(groups * Mg, 3, generator=g)).to(DEV)
    h2, g32, g16 = ops.encoder_stage1(nb, w["w1b1"], w["W2"], w["b2"], groups, Mg)
    a1 = torch.relu(nb.double() @ w["w1b1"][:, :3].double().T + w["w1b1"][:, 3].double()).float().bfloat16()
    ref = a1.double() @ w["W2"].double().T + w["b2"].double()
    scale = ref.abs().mean().item()
    # conv1 outputs that straddle a bf16 rounding boundary move one input by 2^-8 relative: tolerance in units of the output scale
    err = (h2.double() - ref).abs()
    assert err.max().item() < 0.03 * scale + 0.01 * ref.abs().max().item() and err.mean().item() < 0.004 * scale, (err.max().item(), err.mean().item(), scale)
    gref = ref.reshape(groups, Mg, 256).amax(1)
    gerr = (g32.double() - gref).abs()
    assert gerr.max().item() < 0.02 * scale + 0.004 * gref.abs().max().item(), (gerr.max().item(), scale)
    # the maxima are taken before the bf16 rounding of h2, and rounding is monotone: bf16(max) == max(bf16)
    assert torch.equal(g32.bfloat16(), h2.reshape(groups, Mg, 256).amax(1))
    assert torch.equal(g16, g32.bfloat16())


# ------------------------------------------------------------------------------------------ scoring
@pytest.mark.parametrize("Q,Nb,D,tile", [(784, 1500, 768, None), (3136, 5000, 128, None), (100, 77, 64, None),
                                          (1000, 2100, 256, "2"), (515, 9000, 320, "2"),
                                          (784, 1500, 768, "5"), (3136, 5000, 192, "5"), (1000, 2100, 256, "5"), (700, 512, 768, "5"),
                                          (515, 9000, 320, "5"), (300, 256, 192, "5"), (260, 1024, 1024, "5"), (513, 2816, 320, "5")])
def test_l2_min_and_rescore(Q, Nb, D, tile, monkeypatch):
    if tile:  # 5 = the two-group 256x256 pipeline (production from Q >= 512); 2 = the lock-step 8-wave 256x256 shape (test build)
        # (5: whole bank tiles only, the remainder rows go through the 128x128 kernel; D < 192 falls back to the 128x128 kernel)
        if tile not in ("0", "5"):
            need_ab_variants(f"CMDIAD_L2_TILE={tile}")
        monkeypatch.setenv("CMDIAD_L2_TILE", tile)
    g = torch.Generator().manual_seed(Q + Nb)
    bank = torch.randn(Nb, D, generator=g)
    q = bank[torch.randint(0, Nb, (Q,), generator=g)] + 0.3 * torch.randn(Q, D, generator=g)
    b16, b32, bsq = ops.normalize_cast(bank.to(DEV), 0.1, 1 / 1.3, want_f32=True)
    q16, q32, qsq = ops.normalize_cast(q.to(DEV), 0.1, 1 / 1.3, want_f32=True)
    np.testing.assert_allclose(b32.cpu().numpy(), ((bank - 0.1) / 1.3).numpy(), rtol=1e-6, atol=1e-6)
    keys = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV))
    mv, mi = ops.l2_rescore(q32, b32, keys)
    ref_v, ref_i = ok.l2_min_argmin(q32.cpu().numpy(), b32.cpu().numpy())
    same = mi.cpu().numpy() == ref_i
    assert same.mean() > 0.995, same.mean()  # bf16 distance GEMM may flip near-ties only
    np.testing.assert_allclose(mv.cpu().numpy()[same], ref_v[same], rtol=1e-5, atol=1e-5)  # exact fp32 re-score
    np.testing.assert_allclose(mv.cpu().numpy(), ref_v, rtol=2e-3, atol=2e-3)  # a flipped tie is still a near-min
    # sharded bank: two halves + integer min over packed keys == single pass
    h = (Nb // 2 + 63) // 64 * 64 if Nb > 200 else Nb // 2
    k2 = ops.new_keys(Q, DEV)
    ops.l2_min_keys(q16, qsq, b16[:h].contiguous(), bsq[:h].contiguous(), k2, row_offset=0)
    k3 = ops.new_keys(Q, DEV)
    ops.l2_min_keys(q16, qsq, b16[h:].contiguous(), bsq[h:].contiguous(), k3, row_offset=h)
    merged = torch.minimum(k2, k3)  # non-negative keys: signed min == unsigned min
    assert torch.equal(merged, keys)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tile", ["0", "2", "5"])
def test_l2_min_all_tiles_identical_keys(tile, dt, monkeypatch):
    """Both operand types of every distance-GEMM formulation (the engine defaults to fp16): all must return IDENTICAL keys on
    the same operands (same start value -(|q|^2 + |b|^2) / 2, same products, same fp32 accumulation order per 64-deep K tile,
    same truncation and lowest-row rule: RowMin in csrc/l2min.hip), and agree with the fp64 argmin up to bf16 near-ties.
    Shapes with several bank tiles per block, a partial last tile (handled by the 128x128 kernel beside variant 5) and a
    ragged query tile."""
    if tile not in ("0", "5"):
        need_ab_variants(f"CMDIAD_L2_TILE={tile}")
    Q, Nb, D = 1100, 2900, 256
    g = torch.Generator().manual_seed(77)
    bank = torch.randn(Nb, D, generator=g)
    q = bank[torch.randint(0, Nb, (Q,), generator=g)] + 0.3 * torch.randn(Q, D, generator=g)
    b16, b32, bsq = ops.normalize_cast(bank.to(DEV), want_f32=True, dtype=dt)
    q16, q32, qsq = ops.normalize_cast(q.to(DEV), want_f32=True, dtype=dt)
    monkeypatch.setenv("CMDIAD_L2_TILE", "0")
    base = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV)).clone()
    monkeypatch.setenv("CMDIAD_L2_TILE", tile)
    keys = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV))
    assert torch.equal(keys, base)
    _, mi = ops.l2_rescore(q32, b32, keys)
    ref_i = torch.cdist(q.double(), bank.double()).argmin(1)
    assert (mi.cpu() == ref_i).float().mean() > 0.97


@pytest.mark.parametrize("tile", ["0", "5"])
def test_l2_min_key_definition_duplicates_and_value(tile, monkeypatch):
    """What a key holds (RowMin, csrc/l2min.hip): the squared distance of the 16-bit operands with its low mantissa bits cut
    (within 2^-18 of the exact value of the rounded operands, plus fp32 accumulation error), and -- rows repeated in the
    library, in other tiles, lanes and ranges -- the LOWEST of equal rows; a query that IS a library row scores zero."""
    monkeypatch.setenv("CMDIAD_L2_TILE", tile)
    Q, Nb, D = 768, 4096 + 70, 256
    g = torch.Generator().manual_seed(5)
    bank = torch.randn(Nb, D, generator=g)
    src = torch.randint(0, 700, (Q,), generator=g)
    # every source row is repeated further down: same tile (+3), next lane group (+4), next 16-block, other tiles / ranges
    for off in (3, 4, 16, 64, 256, 1024, 2700):
        bank[src + off + 700] = bank[src]       # (copies may overwrite each other: all that matters is that rows >= 703 repeat rows < 700)
    q = bank[src].clone()
    q[Q // 2:] += 0.2 * torch.randn(Q - Q // 2, D, generator=g)
    b16, b32, bsq = ops.normalize_cast(bank.to(DEV), want_f32=True, dtype=torch.float16)
    q16, q32, qsq = ops.normalize_cast(q.to(DEV), want_f32=True, dtype=torch.float16)
    keys = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV))
    val, idx = ops.unpack_keys(keys)
    # the first occurrence of the row is src itself (the copies sit at >= 703; rows below 700 are distinct)
    assert torch.equal(idx.cpu()[:Q // 2], src[:Q // 2]), "a repeated row must resolve to its lowest index"
    assert float(val[:Q // 2].max()) <= 2e-3, "a query that is a library row is at distance ~0 (clamped at 0)"
    # value: d2 of the ROUNDED operands in float64, for the row the key names
    d2 = (q16.double() - b16[idx].double()).pow(2).sum(1)
    np.testing.assert_allclose(val.double().cpu().numpy(), d2.cpu().numpy(), rtol=2e-5, atol=2e-3)
    assert (val >= 0).all()


def _near_tie_library(Nb, D, n_pairs, seed, eps=1e-2):
    """A library in which n_pairs rows have a NEAR-duplicate at a random other place (row + eps * noise: the two are ~eps * sqrt(D)
    apart, inside what 16-bit operands resolve), and queries that sit next to such pairs: the 16-bit search picks the twin
    in a third to a half of the cases."""
    g = torch.Generator().manual_seed(seed)
    bank = torch.randn(Nb, D, generator=g)
    perm = torch.randperm(Nb, generator=g)
    a, b = perm[:n_pairs], perm[n_pairs:2 * n_pairs]
    bank[b] = bank[a] + eps * torch.randn(n_pairs, D, generator=g)
    return bank, a, g


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_l2_runner_up_makes_the_argmin_exact(dt):
    """features.py:227 is torch.min on the fp32 distance matrix: index work.  The 16-bit distance GEMM alone resolves near-ties the
    wrong way (here: about half of the planted ones); with the runner-up of every query (keys [2, Q], include/cmdiad_hip.h) and
    the fp32 decision between the two (cmdiad_l2_rescore2) min_idx equals the fp32 brute-force argmin on >= 99.99 % of the rows
    -- VERDICT round 5 item 2 -- and min_val is its distance."""
    Q, Nb, D = 8192, 6000, 768
    bank, a, g = _near_tie_library(Nb, D, 2000, 11)
    q = bank[a[torch.randint(0, a.shape[0], (Q,), generator=g)]] + 0.3 * torch.randn(Q, D, generator=g)
    b16, b32, bsq = ops.normalize_cast(bank.to(DEV), want_f32=True, dtype=dt)
    q16, q32, qsq = ops.normalize_cast(q.to(DEV), want_f32=True, dtype=dt)
    d = torch.cdist(q32.double(), b32.double())   # brute force over the fp32 rows (features.py:186-190,227), ties-free in float64
    rv, ri = d.min(1)
    k1 = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV))
    _, mi1 = ops.l2_rescore(q32, b32, k1)
    k2 = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV, runner=True))
    mv, mi = ops.l2_rescore(q32, b32, k2)
    one, two = (mi1 == ri).float().mean().item(), (mi == ri).float().mean().item()
    print(f"[argmin == fp32 brute force: winner only {one:.4f}, winner + runner-up {two:.5f}]")
    assert torch.equal(k2[0], k1), "the best plane is the single-plane search"
    assert one < (0.97 if dt == torch.bfloat16 else 0.998), "the planted near-ties must actually defeat the 16-bit search (else this test shows nothing)"
    # >= 99.99 % identical rows; a different row is admissible only as a tie at fp32 resolution
    diff = mi != ri
    assert two >= 0.9995 and bool(((d[diff, mi[diff]] - rv[diff]) <= 2e-7 * rv[diff]).all()), (two, d[diff, mi[diff]] - rv[diff])
    exact = (q32.double() - b32[mi].double()).pow(2).sum(1).sqrt()
    np.testing.assert_allclose(mv.cpu().numpy(), exact.float().cpu().numpy(), rtol=1e-5, atol=1e-5)
    dmin = (q32[:, None, :].double()[:64] - b32[None].double()).pow(2).sum(-1).sqrt().min(1).values   # float64, a sample
    np.testing.assert_allclose(mv[:64].cpu().numpy(), dmin.float().cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tile", ["0", "2", "5"])
def test_l2_runner_up_is_a_property_of_the_library_rows(tile, dt, monkeypatch):
    """The runner-up's definition names library rows only -- the nearest row outside the winner's group of 16 rows,
    group(row) = (row >> 6, (row >> 2) & 3) -- so every formulation returns the same [2, Q] keys, a row-sharded search merged
    with engine.merge_key_planes equals the single-library search on BOTH planes (shards cut at multiples of 64, ragged last
    tiles through the 128-column kernel), and a counted launch equals the plain one on its live rows."""
    if tile not in ("0", "5"):
        need_ab_variants(f"CMDIAD_L2_TILE={tile}")
    Q, Nb, D = 1100, 2900, 256
    bank, a, g = _near_tie_library(Nb, D, 600, 7)
    q = bank[a[torch.randint(0, a.shape[0], (Q,), generator=g)]] + 0.3 * torch.randn(Q, D, generator=g)
    b16, b32, bsq = ops.normalize_cast(bank.to(DEV), want_f32=True, dtype=dt)
    q16, q32, qsq = ops.normalize_cast(q.to(DEV), want_f32=True, dtype=dt)
    monkeypatch.setenv("CMDIAD_L2_TILE", "0")
    base = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV, runner=True)).clone()
    monkeypatch.setenv("CMDIAD_L2_TILE", tile)
    keys = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV, runner=True))
    assert torch.equal(keys, base)
    v, i = ops.unpack_keys(keys)
    grp = lambda r: torch.stack([r >> 6, (r >> 2) & 3])        # noqa: E731
    assert bool((grp(i[0]) != grp(i[1])).any(0).all()), "the runner-up lies outside the winner's group of 16 rows"
    assert bool((keys[1] > keys[0]).all())
    # it IS the nearest outside that group: squared distances of the rounded operands in float64 against the key's value
    d2 = (q16.double()[:, None, :] - b16.double()[None]).pow(2).sum(-1)
    rows = torch.arange(Nb, device=DEV)
    same_group = (grp(rows)[:, None, :] == grp(i[0])[:, :, None]).all(0)
    d2_out = d2.masked_fill(same_group, float("inf"))
    np.testing.assert_allclose(v[1].double().cpu().numpy(), d2_out.min(1).values.cpu().numpy(), rtol=2e-5, atol=2e-3)
    close = d2_out.gather(1, i[1][:, None]).squeeze(1) <= d2_out.min(1).values * (1 + 2e-5) + 2e-3
    assert bool(close.all())
    # three shards (cuts at multiples of 64, a ragged last one) merged == the single library, both planes
    merged = None
    for lo, hi in ((0, 1024), (1024, 2112), (2112, Nb)):
        k = ops.l2_min_keys(q16, qsq, b16[lo:hi].contiguous(), bsq[lo:hi].contiguous(), ops.new_keys(Q, DEV, runner=True), row_offset=lo)
        merged = k if merged is None else eng.merge_key_planes(merged, k)
    assert torch.equal(merged, base)
    # counted launch: the first 777 rows only
    cnt = torch.tensor([777], dtype=torch.int32, device=DEV)
    kc = ops.l2_min_keys_counted(q16, qsq, cnt, b16, bsq, ops.new_keys(Q, DEV, runner=True))
    assert torch.equal(kc[:, :777], base[:, :777]) and bool((kc[:, 777:] == ops.KEY_EMPTY).all())
    with pytest.raises(Exception, match="row_offset"):
        ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV, runner=True), row_offset=100)


def test_l2_non_finite_rows_cannot_win_and_find_nothing():
    """the running minimum compares accumulator bit patterns as unsigned integers, where +NaN / +inf sort below
    every finite candidate.  cmdiad_normalize_cast (the only producer of the search operands) turns a row with a non-finite
    element into zeros with squared norm +inf: as a library row it never wins, as a query it finds nothing (keys untouched); the
    other rows' keys are what the search without those rows returns."""
    Q, Nb, D = 600, 3000, 256
    g = torch.Generator().manual_seed(3)
    bank = torch.randn(Nb, D, generator=g)
    q = bank[torch.randint(0, Nb, (Q,), generator=g)] + 0.3 * torch.randn(Q, D, generator=g)
    bad_b = torch.tensor([0, 17, 255, 256, 1500, Nb - 1])
    bank_bad = bank.clone()
    bank_bad[bad_b[::2], 5] = float("nan")
    bank_bad[bad_b[1::2], 200] = float("inf")
    q_bad = q.clone()
    q_bad[3, 0] = float("nan"); q_bad[300, 9] = float("-inf")
    for dt in (torch.bfloat16, torch.float16):
        b16, _, bsq = ops.normalize_cast(bank_bad.to(DEV), dtype=dt)
        q16, _, qsq = ops.normalize_cast(q_bad.to(DEV), dtype=dt)
        assert bool(torch.isinf(bsq[bad_b.to(DEV)]).all()) and bool((b16[bad_b.to(DEV)].float() == 0).all())
        assert bool(torch.isfinite(b16.float()).all()) and bool(torch.isfinite(q16.float()).all())
        keep = torch.ones(Nb, dtype=torch.bool); keep[bad_b] = False
        rows = keep.nonzero().flatten().to(DEV)
        for tile in ("0", "5"):
            os.environ["CMDIAD_L2_TILE"] = tile
            try:
                keys = ops.l2_min_keys(q16, qsq, b16, bsq, ops.new_keys(Q, DEV, runner=True))
            finally:
                del os.environ["CMDIAD_L2_TILE"]
            _, idx = ops.unpack_keys(keys)
            live = torch.ones(Q, dtype=torch.bool, device=DEV); live[3] = live[300] = False
            assert bool((keys[:, ~live] == ops.KEY_EMPTY).all()), "a non-finite query row finds nothing"
            assert not bool(torch.isin(idx[:, live], bad_b.to(DEV)).any()), "a non-finite library row never wins"
            # the best plane equals the search of the library WITHOUT those rows (row numbers mapped back)
            ref = ops.l2_min_keys(q16, qsq, b16[rows].contiguous(), bsq[rows].contiguous(), ops.new_keys(Q, DEV))
            rv, ri = ops.unpack_keys(ref)
            v, _ = ops.unpack_keys(keys[0])
            assert torch.equal(rows[ri[live]], idx[0][live]) and torch.equal(rv[live], v[live])


def _exact_top3(probes, bank):
    # explicit differences in float64 (torch.cdist's |a|^2 + |b|^2 - 2ab form reports 1e-6 for identical rows even in double)
    d = torch.stack([(bank.double() - p.double()).pow(2).sum(1).sqrt() for p in probes])
    return torch.topk(d, min(3, bank.shape[0]), largest=False)


def test_reweight_scan_top3():
    g = torch.Generator().manual_seed(3)
    bank = torch.randn(4000, 768, generator=g)
    probes = bank[[5, 1234, 3999]].clone()
    top3 = ops.reweight_scan(probes.to(DEV), bank.to(DEV))
    val, idx = ops.unpack_keys(top3)
    rv, ri = _exact_top3(probes, bank)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri.numpy())
    np.testing.assert_allclose(val.sqrt().cpu().numpy(), rv.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("Nb,D,R", [(4001, 768, 32), (16, 768, 1), (37, 256, 5), (20000, 768, 32), (5, 128, 2)])
def test_reweight_scan_shapes_and_block16_layout(Nb, D, R):
    """cmdiad_reweight_scan (fp32 MFMA scan over the block16 copy + exact re-evaluation of 4 candidates) against an exact
    float64 top-3: ragged library sizes (Nb % 16 != 0, Nb < 16), every probe count class, several feature widths; probes
    are library rows (distance 0 to themselves, as m_star always is, features.py:233) and unseen rows."""
    g = torch.Generator().manual_seed(Nb + R)
    bank = torch.randn(Nb, D, generator=g)
    probes = torch.cat([bank[torch.randint(0, Nb, (R - R // 2,), generator=g)], torch.randn(R // 2, D, generator=g)])
    blk = ops.bank_block16(bank.to(DEV))
    # layout: [group][t][kq][row j][4] with k = 16 t + 4 kq + e
    T, G = D // 16, (Nb + 15) // 16
    padded = torch.zeros(G * 16, D)
    padded[:Nb] = bank
    want = padded.view(G, 16, T, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1)
    assert torch.equal(blk.cpu(), want)
    top3 = ops.reweight_scan(probes.to(DEV), bank.to(DEV), blk)
    val, idx = ops.unpack_keys(top3)
    rv, ri = _exact_top3(probes, bank)
    k = ri.shape[1]
    np.testing.assert_array_equal(idx[:, :k].cpu().numpy(), ri.numpy())
    np.testing.assert_allclose(val[:, :k].sqrt().cpu().numpy(), rv.numpy(), rtol=1e-5, atol=1e-5)
    if k < 3:
        assert (top3[:, k:] == ops.KEY_EMPTY).all()


@pytest.mark.parametrize("Nb0,Nb1,R0,R1", [(76518, 19129, 32, 32), (4001, 37, 32, 5), (16, 20000, 1, 32), (300, 300, 7, 7)])
def test_reweight_scan_pair_equals_two_calls(Nb0, Nb1, R0, R1):
    """cmdiad_reweight_scan_pair (the two libraries of a scored batch in ONE launch pair, the scan kernel's workgroups shared in
    proportion to the rows) returns what two cmdiad_reweight_scan calls return, bit for bit -- the bench's library sizes, a
    tiny second library, a tiny first one, equal ones -- and the exact float64 top-3."""
    D = 768
    g = torch.Generator().manual_seed(Nb0 + Nb1)
    banks = [torch.randn(n, D, generator=g) for n in (Nb0, Nb1)]
    probes = [torch.cat([b[torch.randint(0, b.shape[0], (r - r // 2,), generator=g)], torch.randn(r // 2, D, generator=g)])
              for b, r in zip(banks, (R0, R1))]
    db = [b.to(DEV) for b in banks]
    blk = [ops.bank_block16(b) for b in db]
    dp = [p.to(DEV) for p in probes]
    t0, t1 = ops.reweight_scan_pair(dp[0], db[0], blk[0], dp[1], db[1], blk[1])
    for t, p, b, k16 in ((t0, dp[0], db[0], blk[0]), (t1, dp[1], db[1], blk[1])):
        assert torch.equal(t, ops.reweight_scan(p, b, k16))
    if Nb0 + Nb1 < 30000:      # (the bench-sized case is covered by the equality above; its float64 reference alone takes 15 s)
        for t, p, b in ((t0, probes[0], banks[0]), (t1, probes[1], banks[1])):
            rv, ri = _exact_top3(p, b)
            np.testing.assert_array_equal(ops.unpack_keys(t)[1][:, :ri.shape[1]].cpu().numpy(), ri.numpy())


def test_reweight_scan_duplicates_near_ties_and_shards():
    """Exact duplicates of the probe row (all-zero background patches are exact duplicates in real libraries) resolve to
    the LOWEST rows like torch.topk on the exact matrix; rows closer together than the scan's approximation error are
    still ordered by their exact distances; two row shards called in turn give the single-call result."""
    g = torch.Generator().manual_seed(11)
    bank = torch.randn(6000, 768, generator=g)
    bank[[100, 2500, 2501, 5999, 17]] = bank[4000].clone()      # six copies of one row
    near = bank[3000].clone()
    bank[3001] = near + 3e-4 * torch.randn(768, generator=g)     # d2 ~ 7e-5, far below the fp32 expansion's error on |b|^2 ~ 768
    bank[3002] = near + 6e-4 * torch.randn(768, generator=g)
    bank[3003] = near + 9e-4 * torch.randn(768, generator=g)
    probes = torch.stack([bank[4000], bank[3000], torch.zeros(768)])
    bank[50:60] = 0.0                                             # duplicate all-zero rows, probe 2 equals them
    top3 = ops.reweight_scan(probes.to(DEV), bank.to(DEV))
    val, idx = ops.unpack_keys(top3)
    assert idx[0].tolist() == [17, 100, 2500] and float(val[0].max()) == 0.0
    assert idx[1].tolist() == [3000, 3001, 3002]
    assert idx[2].tolist() == [50, 51, 52] and float(val[2].max()) == 0.0
    rv, _ = _exact_top3(probes, bank)
    np.testing.assert_allclose(val.sqrt().cpu().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
    # shards in turn: rows [0, 2560) then [2560, 6000)
    b = bank.to(DEV)
    t2 = ops.reweight_scan(probes.to(DEV), b[:2560].contiguous())
    t2 = ops.reweight_scan(probes.to(DEV), b[2560:].contiguous(), top3=t2, row_offset=2560)
    assert torch.equal(t2, top3)



def test_reweight_scan_clustered_near_duplicates():
    """ADVICE (round 2): libraries built without a coreset hold clusters of near-identical patches.  Clusters of 3-8 rows
    within d2 ~ 1e-5 ... 1e-3 of their centre -- far inside the norm-expansion's ~1e-4 error on |b|^2 = 768 -- probed with
    the centre itself: the three smallest EXACT distances and their rows must be what an exact scan of the library returns
    (the scan keeps 8 approximate candidates per probe and re-evaluates them exactly)."""
    g = torch.Generator().manual_seed(23)
    bank = torch.randn(9000, 768, generator=g)
    probes = []
    for c, size in enumerate((3, 4, 5, 6, 7, 8, 8, 6, 5, 4, 3, 8)):
        centre = torch.randn(768, generator=g)
        rows = torch.randperm(9000, generator=g)[:size]                      # scattered over row residues and groups
        for j, r in enumerate(rows.tolist()):
            bank[r] = centre + (1e-4 * (1 + j) * (1 + c % 3)) * torch.randn(768, generator=g)
        probes.append(centre)
    probes = torch.stack(probes)
    top3 = ops.reweight_scan(probes.to(DEV), bank.to(DEV))
    val, idx = ops.unpack_keys(top3)
    d2 = torch.stack([(bank.double() - p.double()).pow(2).sum(1) for p in probes])
    rv, ri = torch.topk(d2, 3, dim=1, largest=False)
    assert torch.equal(idx.cpu(), ri), (idx.cpu(), ri)
    np.testing.assert_allclose(val.cpu().numpy(), rv.float().numpy(), rtol=2e-5, atol=1e-12)

def test_l2_dist_matrix_exact():
    g = torch.Generator().manual_seed(12)
    q, bank = torch.randn(130, 768, generator=g), torch.randn(333, 768, generator=g)
    q[7] = bank[21]
    d = ops.l2_dist_matrix(q.to(DEV), bank.to(DEV)).cpu()
    ref = torch.stack([(bank.double() - r.double()).pow(2).sum(1).sqrt() for r in q])   # (cdist's expansion is not exact at 0)
    assert float(d[7, 21]) == 0.0
    np.testing.assert_allclose(d.numpy(), ref.numpy(), rtol=2e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------ small ops
def test_im2col_assemble_bilinear_transpose():
    g = torch.Generator().manual_seed(9)
    rgb = torch.randn(2, 3, 224, 224, generator=g)
    pat = ops.im2col_patch8(rgb.to(DEV))
    ref = torch.nn.functional.unfold(rgb, 8, stride=8).transpose(1, 2).reshape(-1, 192)
    np.testing.assert_array_equal(pat.float().cpu().numpy(), _bf(ref).numpy())
    po, cls, pos = torch.randn(2 * 784, 768, generator=g), torch.randn(768, generator=g), torch.randn(785, 768, generator=g)
    tok = ops.vit_assemble(po.to(DEV), cls.to(DEV), pos.to(DEV), 2, 784, 768)
    want = torch.cat([cls.expand(2, 1, 768), po.view(2, 784, 768)], 1) + pos
    np.testing.assert_array_equal(tok.view(2, 785, 768).cpu().numpy(), want.numpy())
    m = torch.rand(3, 56, 56, generator=g)
    up = ops.bilinear_up(m.to(DEV), 224)
    want = torch.nn.functional.interpolate(m[:, None], size=(224, 224), mode="bilinear")[:, 0]
    np.testing.assert_allclose(up.cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(up[0].cpu().numpy(), ok.bilinear_up(m[0].numpy(), 224), rtol=1e-6, atol=1e-7)
    t = torch.randn(130, 70, generator=g).bfloat16()
    np.testing.assert_array_equal(ops.transpose_bf16(t.to(DEV)).float().cpu().numpy(), t.float().T.numpy())


# ------------------------------------------------------------------------------------------ on-device scorer tail (f3)
@pytest.mark.parametrize("n,H,W,radius", [(5, 224, 224, 4.0), (3, 64, 80, 4.0), (2, 100, 37, 1.5), (1, 256, 256, 7.3)])
def test_blur8_maps_bit_exact(n, H, W, radius):
    """cmdiad_blur8_maps vs the reference's KNNGaussianBlur arithmetic: quantisation in torch as utils/utils.py:81-82
    does it, Pillow's blur from the C oracle (pinned to Pillow itself on the CPU) -- every output element identical."""
    g = torch.Generator().manual_seed(n * H + W)
    maps = torch.rand(n, H, W, generator=g) ** 2 * 3.7
    maps[0, : H // 2] *= 0.01
    if n > 1:
        maps[1] = torch.linspace(0, 1, H * W).reshape(H, W)  # many values that sit on a quantisation boundary
    out = ops.blur8_maps(maps.to(DEV), radius).cpu()
    for i in range(n):
        mx = maps[i].max()
        u8 = (maps[i] / mx).mul(255).byte().numpy()
        ref = torch.from_numpy(ok.pil_gaussian_blur_u8(u8, radius)).float().div(255) * mx
        np.testing.assert_array_equal(out[i].numpy(), ref.numpy())


def test_knn_gaussian_blur_vs_reference_golden(golden):
    """The drop-in KNNGaussianBlur (device kernel) against the output of the REFERENCE's own KNNGaussianBlur
    (utils/utils.py:71-83 with real Pillow; tests/golden/g4_score.npz) -- identical bits."""
    from cmdiad_amd.utils.utils import KNNGaussianBlur
    g = golden("g4_score.npz")
    gen = torch.Generator().manual_seed(int(g["blur_seed"]))
    smooth = torch.nn.functional.interpolate(torch.rand(1, 1, 56, 56, generator=gen) * 3.0, size=(224, 224), mode="bilinear")
    out = KNNGaussianBlur(4)(smooth.to(DEV))
    assert out.device.type == "cpu" and out.shape == (1, 224, 224)
    np.testing.assert_array_equal(out.numpy()[:, ::2, ::2], g["blur_out"])
    np.testing.assert_array_equal(KNNGaussianBlur(4)(smooth).numpy(), out.numpy())  # CPU input: moved to the device


def test_blur8_maps_rejects_short_lines():
    from cmdiad_amd._native import NativeError
    with pytest.raises(NativeError):
        ops.blur8_maps(torch.rand(1, 6, 224, device=DEV), 4.0)


def test_ocsvm_score_maps_vs_sklearn():
    """cmdiad_ocsvm_score_maps vs SGDOneClassSVM.score_samples (features.py:114-115, 352-358; call site
    multiple_features.py:985-992) on lambda-weighted map pairs."""
    from sklearn import linear_model
    g = torch.Generator().manual_seed(3)
    maps = torch.rand(3, 2, 224 * 224, generator=g) * torch.tensor([2.0, 20.0]).view(1, 2, 1)
    lam = (1.0, 0.1)
    X = torch.stack([lam[0] * maps[:, 0], lam[1] * maps[:, 1]], -1).reshape(-1, 2)  # as the reference builds s_map
    svm = linear_model.SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000).fit(X[::7])
    want = svm.score_samples(X).reshape(3, -1)
    got = ops.ocsvm_score_maps(maps.to(DEV), lam, svm.coef_, svm.offset_).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)  # f64 dot of two terms: summation order only


# ------------------------------------------------------------------------------------------ edge cases of the point-cloud front end
def test_full_frame_cloud_maximum_size():
    """Every pixel valid: N = 224*224 = 50 176, the largest cloud the path can see (FPS memory-resident fallback)."""
    pc = synth_cloud(21, 3.0)  # ellipse larger than the frame -> no background
    xyz, nz, pix2pt, nv = ops.unorganize(pc.to(DEV))
    assert int(nv[0]) == 224 * 224 and torch.equal(nz[0].cpu(), torch.arange(224 * 224, dtype=torch.int32))
    pts = xyz.cpu().numpy()
    idx, cen = ops.fps(xyz, 256)
    idx_ref, cen_ref = ok.fps(pts, 256)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_ref)
    gi, nb = ops.knn_group(xyz, cen, 128)
    ir, nr = ok.knn_group(pts, cen_ref, 128)
    np.testing.assert_array_equal(gi.cpu().numpy(), ir)
    np.testing.assert_array_equal(nb.cpu().numpy(), nr)


def test_tiny_clouds():
    """Fewer points than groups (FPS then repeats points: every running minimum is 0 and the lowest index wins) and
    exactly K points (the neighbourhood is the whole cloud); K > N is rejected."""
    from cmdiad_amd._native import NativeError
    xyz, _ = _cloud(22, 0.05)
    few = np.ascontiguousarray(xyz[:40])
    idx, cen = ops.fps(torch.from_numpy(few[None]).to(DEV), 64)
    idx_ref, cen_ref = ok.fps(few[None], 64)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_ref)
    np.testing.assert_array_equal(cen.cpu().numpy(), cen_ref)
    gi, nb = ops.knn_group(torch.from_numpy(few[None]).to(DEV), cen, 40)
    ir, nr = ok.knn_group(few[None], cen_ref, 40)
    np.testing.assert_array_equal(gi.cpu().numpy(), ir)
    np.testing.assert_array_equal(nb.cpu().numpy(), nr)
    assert all(sorted(row) == list(range(40)) for row in gi[0].cpu().tolist())
    with pytest.raises(NativeError):
        ops.knn_group(torch.from_numpy(few[None]).to(DEV), cen, 41)


def test_empty_frame_is_reported():
    """An all-background frame has no points: unorganize reports n = 0 and the drop-in raises instead of sampling."""
    pc = torch.zeros(1, 3, 224, 224)
    xyz, nz, pix2pt, nv = ops.unorganize(pc.to(DEV))
    assert int(nv[0]) == 0 and bool((pix2pt == -1).all())


# ------------------------------------------------------------------------------------------ pointnet2_ops / knn_cuda surface (f4)
@pytest.mark.parametrize("radius,nsample", [(0.004, 16), (0.02, 64), (0.0005, 8)])
def test_ball_query_bit_exact(radius, nsample):
    a, _ = _cloud(31, 0.08)
    b, _ = _cloud(32, 0.06)
    N = min(len(a), len(b))
    xyz = np.stack([a[:N], b[:N]])
    cen = np.stack([ok.fps(a[None, :N], 100)[1][0], ok.fps(b[None, :N], 100)[1][0]])
    cen[0, 7] += 1.0  # a query with nothing in range -> zeros
    ref = ok.ball_query(radius, nsample, xyz, cen)
    got = ops.ball_query(radius, nsample, torch.from_numpy(xyz).to(DEV), torch.from_numpy(cen).to(DEV))
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    assert (ref[0, 7] == 0).all()


def test_reference_models_run_on_compat_shims():
    """pointnet2_ops.pointnet2_utils / knn_cuda stand-ins: the wheel's call signatures (models/models.py:70-113 usage) give
    the same indices and gathers as the C oracle; QueryAndGroup = ball query + gather + centre subtraction."""
    from cmdiad_amd.compat import knn_cuda, pointnet2_utils as p2
    a, _ = _cloud(33, 0.1)
    xyz = torch.from_numpy(a[None]).to(DEV)
    idx = p2.furthest_point_sample(xyz, 128)
    assert idx.dtype == torch.int32
    idx_ref, cen_ref = ok.fps(a[None], 128)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_ref)
    center = p2.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()  # models.py:76-77
    np.testing.assert_array_equal(center.cpu().numpy(), cen_ref)
    dist, nn_idx = knn_cuda.KNN(k=32, transpose_mode=True)(xyz, center)                                # models.py:86,100
    ir, nr = ok.knn_group(a[None], cen_ref, 32)
    assert nn_idx.dtype == torch.int64
    np.testing.assert_array_equal(nn_idx.cpu().numpy(), ir)
    np.testing.assert_allclose(dist.cpu().numpy(), np.sqrt((nr ** 2).sum(-1)), rtol=1e-6)
    g = p2.QueryAndGroup(0.01, 24)(xyz, center)
    bq = ok.ball_query(0.01, 24, a[None], cen_ref)
    want = a[bq[0]] - cen_ref[0][:, None, :]                                                            # [M,ns,3]
    np.testing.assert_array_equal(g[0].permute(1, 2, 0).cpu().numpy(), want)


@pytest.mark.parametrize("Mg,groups", [(128, 24), (64, 9), (32, 7), (32, 50), (128, 300), (128, 770), (64, 1031), (32, 2051)])
def test_encoder_tail_equals_two_kernel_path(Mg, groups):
    """cmdiad_encoder_tail (h3 produced and consumed in LDS) against cmdiad_gemm_bf16(ReLU, group bias) + cmdiad_gemm_groupmax:
    the same bf16 rounding of h3 and the same K order of the fp32 accumulation -> identical tokens, for every group size
    (blocks of 128 rows hold one, two or four groups), a ragged last block, and one to four row tiles per persistent block
    (256 blocks walk the tiles: the weight stream, the next tile's h2 and the maxima of the finished tile overlap)."""
    from oracle import nets
    from cmdiad_amd.runtime import fold_pointmae_encoder
    w = fold_pointmae_encoder(nets.synth_state_dict("pointmae", 21), "encoder.", DEV)
    g = torch.Generator().manual_seed(Mg + groups)
    h2 = torch.randn(groups * Mg, 256, generator=g).to(DEV).bfloat16()
    gb = torch.randn(groups, 512, generator=g).to(DEV)
    _, h3 = ops.gemm(h2, w["W3b"], act=ops.ACT_RELU, group_bias=gb, group_rows=Mg)
    want, _ = ops.gemm_groupmax(h3, w["W4"], w["b4"], groups, Mg)
    got = ops.encoder_tail(h2, gb, w["W3b"], w["W4"], w["b4"], groups, Mg)
    assert torch.equal(got, want)


def test_gemm_device_row_count_and_rows_expand():
    """cmdiad_gemm_bf16 with m_count (ABI 2): a launch sized for M rows computes and stores only the first *m_count of them (both
    the 128 x 128 kernel and the persistent 256 x 256 kernel), bit-identical to a launch of exactly that many rows, and leaves
    the other output rows untouched; cmdiad_rows_expand_f32 puts compacted per-row results back on every original row."""
    g = torch.Generator().manual_seed(41)
    M, K = 3000, 256
    A = torch.randn(M, K, generator=g).to(DEV).bfloat16()
    for N in (1920, 768, 2048):
        W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).bfloat16()
        bias = torch.randn(N, generator=g).to(DEV)
        for live in (0, 1, 129, 1537, 2999, 3000, 5000):
            cnt = torch.tensor([live], dtype=torch.int32, device=DEV)
            n = min(live, M)
            for env in ("0", "1"):
                os.environ["CMDIAD_GEMM_PP3"] = env
                try:
                    o16 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
                    o32 = torch.full((M, N), 7.0, dtype=torch.float32, device=DEV)
                    if env == "1" and N % 256 == 0:
                        ops.gemm(A, W, bias=bias, act=ops.ACT_GELU, out_bf16=o16, m_count=cnt)                 # persistent kernel: bf16 only
                        _, want = ops.gemm(A[:max(n, 1)], W, bias=bias, act=ops.ACT_GELU)
                        assert torch.equal(o16[:n], want[:n]) and bool((o16[n:] == 7.0).all()), (N, live, env)
                    else:
                        ops.gemm(A, W, bias=bias, act=ops.ACT_GELU, out_f32=o32, out_bf16=o16, m_count=cnt)
                        want32, want16 = ops.gemm(A[:max(n, 1)], W, bias=bias, act=ops.ACT_GELU, want_f32=True)
                        assert torch.equal(o32[:n], want32[:n]) and torch.equal(o16[:n], want16[:n]), (N, live, env)
                        assert bool((o32[n:] == 7.0).all()) and bool((o16[n:] == 7.0).all()), (N, live, env)
                finally:
                    del os.environ["CMDIAD_GEMM_PP3"]
    rows = torch.randn(37, 768, generator=g).to(DEV)
    slot = torch.randint(0, 37, (500,), generator=g).int().to(DEV)
    assert torch.equal(ops.rows_expand_f32(rows, slot), rows[slot.long()])
