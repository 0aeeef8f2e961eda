"""Float64 restatement of the reference's point-cloud -> patch-grid chain (models/pointnet2_utils.py:72 and features.py:169-184),
the yardstick of csrc/interp_pool.hip's interp_gather and xyz_patch_fused kernels.  TEST INFRASTRUCTURE ONLY: torch CPU operators
in float64, the reference's own composition (gather, scatter into a zero map, AvgPool2d(3, 1), AdaptiveAvgPool2d, normalise), no
code shared with cmdiad_amd.  Proved against torch's fp32 operators and the C oracle in tests/test_patch_ref_cpu.py.

Besides the value it returns, per output element, the ABSOLUTE sum  A = sum |coef * w| * |f|  of the same linear map (the chain
run on |w|, |f|: every pooling coefficient is positive), which is what a rounding-error bound of a sum is proportional to, and
the number of (pixel, neighbour) entries n_e in each patch's footprint, the length of the longest chain of roundings."""
import numpy as np
import torch
import torch.nn.functional as F


def _t64(x):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().to(torch.float64)


def _tl(x):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().long()


def interp_gather(feat, idx3, w3):
    """feat [S, D], idx3 [N, 3], w3 [N, 3] -> (out [N, D], absolute sum [N, D]) in float64: sum_k w3[n, k] * feat[idx3[n, k]]."""
    f, w, i = _t64(feat), _t64(w3), _tl(idx3)
    g = f[i]                                              # [N, 3, D]
    return (g * w.unsqueeze(-1)).sum(1), (g.abs() * w.abs().unsqueeze(-1)).sum(1)


def footprint_entries(size, P):
    """[P*P] int: n_e = 3 * (rows) * (columns) of the size x size map that a patch reads: its adaptive bin over the (size-2)^2
    pooled map, widened by the 3 x 3 window."""
    L = size - 2
    lo = np.arange(P) * L // P
    hi = -((-(np.arange(P) + 1) * L) // P)                # ceil((p + 1) L / P)
    ext = hi - lo + 2
    return (3 * ext[:, None] * ext[None, :]).reshape(-1)


def footprint_windows(size, P):
    """-> (y0, y1, x0, x1) arrays [P*P]: the patch reads map rows [y0, y1) and columns [x0, x1)."""
    L = size - 2
    lo = np.arange(P) * L // P
    hi = -((-(np.arange(P) + 1) * L) // P) + 2
    y0, x0 = np.meshgrid(lo, lo, indexing="ij")
    y1, x1 = np.meshgrid(hi, hi, indexing="ij")
    return y0.reshape(-1), y1.reshape(-1), x0.reshape(-1), x1.reshape(-1)


def _chain(interp, pts, pix, size, P):
    D = interp.shape[1]
    full = torch.zeros((1, D, size * size), dtype=interp.dtype)
    full[0][:, pix] = interp[pts].T                        # the reference's full[:, :, nonzero_indices] = interpolated_pc
    pooled = F.adaptive_avg_pool2d(F.avg_pool2d(full.view(1, D, size, size), 3, stride=1), (P, P))
    return pooled.reshape(D, -1).T


def xyz_patch(feat, idx3, w3, pix2pt, size, P, mean=0.0, inv_std=1.0):
    """One cloud.  feat [S, D], idx3 / w3 [N, 3] (rows that no pixel names are ignored), pix2pt [size*size] int (-1: background)
    -> (patch [P*P, D] float64 = (pooled - mean) * inv_std, A [P*P, D] float64 = the absolute sum BEFORE normalisation,
        n_e [P*P] int)."""
    p2p = _tl(pix2pt).reshape(-1)
    assert p2p.numel() == size * size
    pix = torch.nonzero(p2p >= 0).reshape(-1)
    pts = p2p[pix]
    val, ab = interp_gather(feat, idx3, w3)
    out = _chain(val, pts, pix, size, P)
    a = _chain(ab, pts, pix, size, P)
    return ((out - float(mean)) * float(inv_std)).numpy(), a.numpy(), footprint_entries(size, P)


def error_bound(ref, A, n_e, inv_std=1.0, bf16=False):
    """The derived bound on |kernel - ref| per element, [P*P, D].
    The kernel's value is a sum of products coef * w * f.  A term passes through at most n_e + 6 fp32 roundings: four for
    coef * w (two divisions, two products), at most (entries folded into its centre) + (centres in the list) <= n_e + 1 additions,
    one product with f -- whatever the order of the sum and whether or not products and additions are fused.  Each is relative
    2^-24 on a partial sum that the absolute sum A bounds, so the sum is within (n_e + 8) * 2^-24 * A of the exact value (8, not 6:
    the second-order terms of (1 + u)^k), and that error is scaled by |inv_std|.  The normalisation adds two roundings of half an
    ulp of (about) the result: one ulp, taken as 2^-23 * |ref|.  A bf16 output is the fp32 one rounded once more: the issue
    allows 2^-8 * |ref| for it (round-to-nearest needs 2^-9)."""
    u = 2.0 ** -24
    b = (np.asarray(n_e, np.float64)[:, None] + 8.0) * u * A * abs(float(inv_std)) + 2.0 ** -23 * np.abs(ref)
    if bf16:
        b = b + 2.0 ** -8 * np.abs(ref)
    return b


def synth_batch(B, size, S, D, seed):
    """Seeded inputs of a ragged batch: organised clouds [B, 3, size, size] f32 with a DIFFERENT foreground per cloud (ellipses of
    different areas; from B >= 3 on, cloud 1 keeps five pixels only and cloud 2 is the full frame), centres [B, S, 3] f32 (random
    pixels of each cloud's full surface) and centre features [B, S, D] f32."""
    from cmdiad_amd.synth import synth_cloud
    g = torch.Generator().manual_seed(1000 + seed)
    pcs, cens = [], []
    for b in range(B):
        surface = synth_cloud(seed * 100 + b, 3.0, size=size)          # frac 3: the ellipse contains the whole frame
        assert bool((surface != 0).all())
        if B >= 3 and b == 1:
            keep = torch.zeros(size * size, dtype=torch.bool)
            keep[torch.randperm(size * size, generator=g)[:5]] = True
            pc = surface * keep.view(1, 1, size, size)
        elif B >= 3 and b == 2:
            pc = surface
        else:
            pc = synth_cloud(seed * 100 + b, 0.15 + 0.07 * ((b * 5) % 11), size=size)
        pcs.append(pc)
        pick = torch.randperm(size * size, generator=g)[:S]
        cens.append(surface[0].reshape(3, -1).T[pick])
    feat = torch.randn(B, S, D, generator=g)
    return torch.cat(pcs, 0).contiguous(), torch.stack(cens, 0).contiguous(), feat
