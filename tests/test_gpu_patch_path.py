"""GPU: the point-cloud -> patch-grid kernels (csrc/interp_pool.hip: interp_gather, xyz_patch_fused) and ops.gather_points against
independent references, at the batch sizes, widths and map sizes where they can go wrong: batches that use the block -> image
remap (B = 3, 8, 9, 11), ragged clouds (a nearly empty one and a full frame among them), D = 1152 (more than one trip of the
channel loop, with a tail), overlapping adaptive bins (P > size - 2), a centre list near the LDS limit, three centres in all.

Yardstick: tests/patch_ref.py (float64, the reference's own chain; proved in tests/test_patch_ref_cpu.py).  idx3 / w3 come from
the project's ops.unorganize / ops.interp3nn (bit-pinned to the C oracle in test_gpu_kernels.py) or are built by hand.
Tolerance: patch_ref.error_bound -- derived there, computed here from the float64 reference; nothing is tuned.
interp_pool.hip is compiled with -ffp-contract=off, so interp_gather is held to the BIT-EQUAL alternative of its check: a numpy
fp32 evaluation of (a*w0 + b*w1) + c*w2 with one rounding per operation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_ref as pr  # noqa: E402
import patch_threads_worker as worker  # noqa: E402
from cmdiad_amd import _native as nat  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gather_np(feat, idx3, w3):
    """fp32, one rounding per operation, the kernel's association."""
    a, b, c = feat[idx3[:, 0]], feat[idx3[:, 1]], feat[idx3[:, 2]]
    w0, w1, w2 = (w3[:, k:k + 1] for k in range(3))
    r = (a * w0 + b * w1) + c * w2
    assert r.dtype == np.float32
    return r


def _check_patch(p32, p16, feat, idx3, w3, pix2pt, size, P, mean, inv_std):
    """One cloud's kernel output against the float64 chain, within the derived bound; -> the float64 reference."""
    ref, A, n_e = pr.xyz_patch(feat, idx3, w3, pix2pt, size, P, mean, inv_std)
    err = np.abs(p32.astype(np.float64) - ref)
    bound = pr.error_bound(ref, A, n_e, inv_std)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (worst, err[worst], bound[worst], ref[worst])
    err16 = np.abs(p16.astype(np.float64) - ref)
    bound16 = pr.error_bound(ref, A, n_e, inv_std, bf16=True)
    worst = np.unravel_index(np.argmax(err16 - bound16), err16.shape)
    assert np.all(err16 <= bound16), (worst, err16[worst], bound16[worst], ref[worst])
    return ref


def _run_batch(B, D, size, P, S, seed, mean, inv_std):
    pcs, cen, feat = pr.synth_batch(B, size, S, D, seed)
    dfeat = feat.to(DEV)
    xyz, _, pix2pt, nv = ops.unorganize(pcs.to(DEV))
    idx3, w3 = ops.interp3nn(xyz, cen.to(DEV), n_valid=nv)
    p32, p16 = ops.xyz_patch_fused(dfeat, idx3, w3, pix2pt, size, P, mean, inv_std, want_bf16=True)
    gat = ops.interp_gather(dfeat, idx3, w3, n_valid=nv)
    n = nv.cpu().tolist()
    assert len(set(n)) == B                                      # a different n_valid per cloud
    if B >= 3:
        assert n[1] == 5 and n[2] == size * size                 # nearly empty; the full frame
    for b in range(B):
        i3, w, p2p = idx3[b].cpu().numpy(), w3[b].cpu().numpy(), pix2pt[b].cpu().numpy()
        _check_patch(p32[b].cpu().numpy(), p16[b].float().cpu().numpy(), feat[b].numpy(), i3, w, p2p, size, P, mean, inv_std)
        g = gat[b].cpu().numpy()
        np.testing.assert_array_equal(g[:n[b]], _gather_np(feat[b].numpy(), i3[:n[b]], w[:n[b]]))
        assert not g[n[b]:].any()                                # rows at or beyond n_valid stay zero
        if B > 1:                                                # batch independence: the B = 1 call on this cloud, bit for bit
            q32, q16 = ops.xyz_patch_fused(dfeat[b:b + 1], idx3[b:b + 1], w3[b:b + 1], pix2pt[b:b + 1], size, P, mean, inv_std, want_bf16=True)
            assert torch.equal(q32[0], p32[b]) and torch.equal(q16[0].view(torch.int16), p16[b].view(torch.int16))
            assert torch.equal(ops.interp_gather(dfeat[b:b + 1], idx3[b:b + 1], w3[b:b + 1], n_valid=nv[b:b + 1])[0], gat[b])


# B, D and (size, P) are factors of one grid: every value once.  (224, 56) / (224, 28): production, footprints of 7 and 10-11;
# (64, 16): bins of 3-4; (30, 28): bins of exactly one pooled pixel; (10, 16): P > size - 2, overlapping bins.  S >= 64 takes
# interp3nn's centre grid, below it the plain scan.  D = 260: one trip of the channel loop with idle lanes; 1152: 2.25 trips at 128
# threads per patch.
@pytest.mark.parametrize("B,D,size,P,S,mean,inv_std", [(1, 4, 224, 56, 256, 0.0, 1.0), (3, 260, 224, 28, 128, 0.25, 1 / 1.7),
                                                      (8, 1152, 30, 28, 64, -3.7, 41.0), (9, 260, 64, 16, 100, -0.4, 2.5),
                                                      (11, 4, 10, 16, 8, 0.1, 1 / 1.3)])
def test_patch_and_gather_grid(B, D, size, P, S, mean, inv_std):
    _run_batch(B, D, size, P, S, seed=B, mean=mean, inv_std=inv_std)


def test_ragged_batch_of_eleven_at_production_width():
    """Two rounds of the eight-image block remap (the second with three images and five idle slots), D = 1152."""
    _run_batch(11, 1152, 64, 16, 70, seed=12, mean=0.05, inv_std=0.8)


def test_footprint_above_twelve_is_an_argument_error():
    pcs, cen, feat = pr.synth_batch(1, 224, 16, 4, seed=1)
    xyz, _, pix2pt, nv = ops.unorganize(pcs.to(DEV))
    idx3, w3 = ops.interp3nn(xyz, cen.to(DEV), n_valid=nv)
    assert pr.footprint_entries(224, 14).max() == 3 * 19 * 19
    with pytest.raises(nat.NativeError, match="footprint 19 exceeds 12"):
        ops.xyz_patch_fused(feat.to(DEV), idx3, w3, pix2pt, 224, 14)


def test_dense_frame_fills_the_centre_list():
    """Every pixel valid at size 96, P 12: footprints of up to 11 x 11 x 3 = 363 entries, and idx3 built BY HAND so that the
    entries of a footprint name (nearly) all different centres -- the fold leaves a list of up to 363 centres (the LDS arrays hold
    432), the rank sort orders it, and the row gather walks it eight at a time with a clamped tail.  (Three nearest centres of
    S <= 4096 real centres cannot do this: 121 pixels would need 363 centres of their own.)"""
    size, P, S, D = 96, 12, 4096, 36
    g = np.random.default_rng(7)
    Y, X = np.divmod(np.arange(size * size), size)
    base = ((Y % 12) * 12 + (X % 12)) * 3                       # distinct over any window of at most 12 x 12 pixels
    idx3 = np.stack([base, base + 1, base + 2], 1)
    rep = (Y * 7 + X * 3) % 5 == 0
    idx3[rep, 2] = idx3[rep, 0]                                 # a fifth of the pixels name a centre twice: the fold has work
    idx3 = ((idx3 * 9 + 5) % S).astype(np.int32)                # injective on [0, 432): spread over the S feature rows
    w3 = g.random((size * size, 3)).astype(np.float32) + 0.05
    w3 /= w3.sum(1, keepdims=True)
    pix2pt = np.arange(size * size, dtype=np.int32)
    feat = g.standard_normal((S, D)).astype(np.float32)
    y0, y1, x0, x1 = pr.footprint_windows(size, P)
    img = idx3.reshape(size, size, 3)
    counts = np.array([len(np.unique(img[y0[p]:y1[p], x0[p]:x1[p]])) for p in range(P * P)])
    assert pr.footprint_entries(size, P).max() == 363 and counts.max() > 300 and np.any(counts % 8 != 0) and counts.max() <= 432
    t = lambda a: torch.from_numpy(a[None]).to(DEV)             # noqa: E731
    p32, p16 = ops.xyz_patch_fused(t(feat), t(idx3), t(w3), t(pix2pt), size, P, 0.3, 1.9, want_bf16=True)
    _check_patch(p32[0].cpu().numpy(), p16[0].float().cpu().numpy(), feat, idx3, w3, pix2pt, size, P, 0.3, 1.9)


def test_three_centres_fold_into_three_entries():
    pcs, cen, feat = pr.synth_batch(1, 64, 3, 8, seed=5)
    xyz, _, pix2pt, nv = ops.unorganize(pcs.to(DEV))
    idx3, w3 = ops.interp3nn(xyz, cen.to(DEV), n_valid=nv)
    n = int(nv[0])
    assert np.array_equal(np.sort(idx3[0, :n].cpu().numpy(), 1), np.tile(np.arange(3), (n, 1)))
    p32, p16 = ops.xyz_patch_fused(feat.to(DEV), idx3, w3, pix2pt, 64, 16, want_bf16=True)
    _check_patch(p32[0].cpu().numpy(), p16[0].float().cpu().numpy(), feat[0].numpy(), idx3[0].cpu().numpy(), w3[0].cpu().numpy(),
                 pix2pt[0].cpu().numpy(), 64, 16, 0.0, 1.0)


def test_empty_window_is_exactly_the_normalised_zero():
    """A patch whose whole window is background: (0 - mean) * inv_std in fp32, exactly, and its bf16 rounding."""
    size, P, mean, inv_std = 224, 56, 0.25, 1 / 1.7
    pcs, cen, feat = pr.synth_batch(1, size, 32, 8, seed=6)
    xyz, _, pix2pt, nv = ops.unorganize(pcs.to(DEV))
    idx3, w3 = ops.interp3nn(xyz, cen.to(DEV), n_valid=nv)
    p32, p16 = ops.xyz_patch_fused(feat.to(DEV), idx3, w3, pix2pt, size, P, mean, inv_std, want_bf16=True)
    valid = (pix2pt[0].cpu().numpy() >= 0).reshape(size, size)
    y0, y1, x0, x1 = pr.footprint_windows(size, P)
    empty = np.array([not valid[y0[p]:y1[p], x0[p]:x1[p]].any() for p in range(P * P)])
    assert 100 < empty.sum() < P * P - 100
    want = (np.float32(0.0) - np.float32(mean)) * np.float32(inv_std)
    assert want.dtype == np.float32
    got = p32[0].cpu().numpy()
    assert np.all(got[empty] == want) and np.all(got[~empty].any(1))
    want16 = torch.tensor([want]).to(torch.bfloat16).view(torch.int16).item()
    assert np.all(p16[0].view(torch.int16).cpu().numpy()[empty] == want16)


def test_threads_per_patch_variants_give_identical_bits(tmp_path):
    """CMDIAD_XYZ_PATCH_THREADS = 64 / 128 / 256 is read once per process: three fresh children (tests/patch_threads_worker.py),
    one after the other, each under a timeout; a child that fails ends the test before the next one starts.  The launcher's
    comment claims identical bits for the three; the default (128) in this process must give them too."""
    outs = {}
    for nt in ("64", "128", "256"):
        env = dict(os.environ, CMDIAD_XYZ_PATCH_THREADS=nt)
        path = str(tmp_path / f"nt{nt}.npz")
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "patch_threads_worker.py"), path], capture_output=True, text=True,
                           timeout=300, env=env, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[nt] = np.load(path)
        assert str(outs[nt]["threads"]) == nt
    for nt in ("128", "256"):
        assert np.array_equal(outs["64"]["p32"].view(np.int32), outs[nt]["p32"].view(np.int32))
        assert np.array_equal(outs["64"]["p16"], outs[nt]["p16"])
    if "CMDIAD_XYZ_PATCH_THREADS" not in os.environ:
        p32, p16 = worker.run_case(DEV)
        assert np.array_equal(p32.view(np.int32), outs["128"]["p32"].view(np.int32)) and np.array_equal(p16, outs["128"]["p16"])


@pytest.mark.parametrize("C", [1, 3, 67])
def test_gather_points_equals_torch_indexing(C):
    """out[b, c, ...] = feat[b, c, idx[b, ...]] for idx [B, M] (gather_operation) and [B, M, K] (grouping_operation): repeated
    indices, index 0 and N - 1, M * K not a multiple of the block."""
    B, N = 3, 1000
    g = torch.Generator().manual_seed(C)
    feat = torch.randn(B, C, N, generator=g)
    for shape in ((B, 301), (B, 37, 9)):
        idx = torch.randint(0, N, shape, generator=g, dtype=torch.int32)
        flat = idx.view(B, -1)
        flat[:, 0], flat[:, 1], flat[:, 2], flat[:, -1] = 0, N - 1, N - 1, 0
        flat[1, 10:40] = 123
        got = ops.gather_points(feat.to(DEV), idx.to(DEV)).cpu()
        want = torch.stack([feat[b][:, idx[b].long()] for b in range(B)])
        assert got.shape == (B, C, *shape[1:]) and torch.equal(got, want)
