"""Tensor-level entry points: torch tensors in (device memory + stream plumbing only),
libcmdiad_hip.so kernels underneath.  Every op raises if the tensors are not on the GPU or the
native library is missing -- there is no eager / CPU fallback here by design.
"""
import ctypes
import math
import os

import torch

from . import _native as nat

ACT_NONE, ACT_GELU, ACT_RELU, ACT_RELU_POST = 0, 1, 2, 3
# cmdiad_loss_head: mode = the row loss + the activation of the network's output (include/cmdiad_hip.h CMDIAD_LOSS_OUT_*; the GELU
# that closes an MlpBlock is the default, SIGMOID applies to the output AND the target)
LOSS_L2, LOSS_COS_DIST, LOSS_SMOOTH_L1 = 0, 1, 2
LOSS_OUT_GELU, LOSS_OUT_NONE, LOSS_OUT_SIGMOID = 0, 256, 512
# "no candidate yet" key: the largest NON-NEGATIVE int64.  Every real key is (fp32 bits of d2 >= +0) << 32 | row, i.e. has bit 63
# clear, so this sentinel is >= every real key under the kernels' unsigned atomicMin AND under the signed MIN all-reduce of the
# row-sharded search (a rank whose shard is empty contributes only sentinels and can never win the reduce).
KEY_EMPTY = 0x7FFFFFFFFFFFFFFF


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Raw HIP stream of torch's current stream.  torch.cuda.current_stream() costs ~100 us per call (availability checks,
    Stream object construction) -- 20 ms per image over the ~600 launches of a B = 1 predict; the raw getters cost < 1 us."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_SHARED_STREAMS = {}


def shared_stream(device, role, priority=0):
    """One HIP stream per (device, role, priority) for the whole process.  torch hands out streams from a pool of 32 per device
    and priority, round robin: objects that each create their own (a predictor per class, a method object per run) walk
    through the pool and end up on the SAME underlying stream as somebody else's -- RCCL's communicator stream, the graph-capture
    stream -- and a capture that forks onto such a stream puts RCCL's events "in a capturing stream": its watchdog thread then
    raises and takes the process down (tools/fuzz_pipeline.py, profiles/r5_notes.md section 15).  Roles are few and fixed."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev.index, role, int(priority))
    st = _SHARED_STREAMS.get(key)
    if st is None:
        st = _SHARED_STREAMS[key] = torch.cuda.Stream(dev, priority=int(priority))
    return st


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise nat.NativeError(f"{name}: tensor must live on the GPU (cmdiad_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")


def _call(name, *args):
    nat.check(getattr(nat.lib(), name)(*args), name)


def _workspace(query_name, device, *args):
    """(uint8 tensor, nbytes) for the library's size query `query_name`(*args).  The tensor holds at least 16 bytes: the _ws entry
    points want a non-null pointer when the size is 0."""
    nbytes = int(getattr(nat.lib(), query_name)(*args))
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device), nbytes


# ------------------------------------------------------------------------------------ point cloud
def fps(xyz, G, n_valid=None):
    """xyz [B,N,3] f32 -> (idx [B,G] int32, centers [B,G,3] f32).  models/models.py:70-78."""
    _chk(xyz, torch.float32, "fps.xyz"); _chk(n_valid, torch.int32, "fps.n_valid")
    B, N, _ = xyz.shape
    idx = torch.empty((B, G), dtype=torch.int32, device=xyz.device)
    cen = torch.empty((B, G, 3), dtype=torch.float32, device=xyz.device)
    ws, wsb = _workspace("cmdiad_fps_workspace_bytes", xyz.device, B, N)
    _call("cmdiad_fps", _p(xyz), _p(n_valid), B, N, G, _p(idx), _p(cen), _p(ws), wsb, _stream())
    return idx, cen


def knn_group(xyz, center, K, n_valid=None, want_idx=True):
    """-> (idx [B,G,K] int64, neighborhood [B,G,K,3] f32).  models/models.py:88-113."""
    _chk(xyz, torch.float32, "knn.xyz"); _chk(center, torch.float32, "knn.center")
    B, N, _ = xyz.shape
    G = center.shape[1]
    idx = torch.empty((B, G, K), dtype=torch.int64, device=xyz.device) if want_idx else None
    nb = torch.empty((B, G, K, 3), dtype=torch.float32, device=xyz.device)
    ws, wsb = _workspace("cmdiad_knn_workspace_bytes", xyz.device, B, N)     # the binned clouds of the neighbourhood search (clouds >= 2 048 points)
    _call("cmdiad_knn_group_ws", _p(xyz), _p(n_valid), _p(center), B, N, G, K, _p(idx), _p(nb), _p(ws), wsb, _stream())
    return idx, nb


def unorganize(organized_pc, n_max=None):
    """organized_pc [B,3,H,W] f32 -> (xyz [B,Nmax,3], nz [B,Nmax] i32, pix2pt [B,HW] i32, n_valid [B] i32).
    multiple_features.py:10-25."""
    _chk(organized_pc, torch.float32, "unorganize.pc")
    B, _, H, W = organized_pc.shape
    HW = H * W
    n_max = n_max or HW
    dev = organized_pc.device
    xyz = torch.zeros((B, n_max, 3), dtype=torch.float32, device=dev)
    nz = torch.zeros((B, n_max), dtype=torch.int32, device=dev)
    pix2pt = torch.empty((B, HW), dtype=torch.int32, device=dev)
    n_valid = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("cmdiad_unorganize", _p(organized_pc), B, HW, n_max, _p(xyz), _p(nz), _p(pix2pt), _p(n_valid), _stream())
    return xyz, nz, pix2pt, n_valid


def ball_query(radius, nsample, xyz, new_xyz, n_valid=None):
    """pointnet2_ops ball_query: xyz [B,N,3], new_xyz [B,M,3] -> idx [B,M,nsample] int32."""
    _chk(xyz, torch.float32, "ball_query.xyz"); _chk(new_xyz, torch.float32, "ball_query.new_xyz")
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = torch.empty((B, M, nsample), dtype=torch.int32, device=xyz.device)
    _call("cmdiad_ball_query", _p(xyz), _p(n_valid), _p(new_xyz), B, N, M, float(radius), int(nsample), _p(idx), _stream())
    return idx


def gather_points(feat, idx):
    """feat [B,C,N] f32, idx [B,...] int32 -> [B,C,...] (gather_operation / grouping_operation)."""
    _chk(feat, torch.float32, "gather.feat"); _chk(idx, torch.int32, "gather.idx")
    B, C, N = feat.shape
    J = idx[0].numel()
    out = torch.empty((B, C, *idx.shape[1:]), dtype=torch.float32, device=feat.device)
    _call("cmdiad_gather_points", _p(feat), _p(idx), B, C, N, J, _p(out), _stream())
    return out


def interp3nn(xyz, center, n_valid=None):
    """-> (idx3 [B,N,3] i32, w3 [B,N,3] f32).  models/pointnet2_utils.py:45-71."""
    _chk(xyz, torch.float32, "interp3nn.xyz"); _chk(center, torch.float32, "interp3nn.center")
    B, N, _ = xyz.shape
    idx3 = torch.zeros((B, N, 3), dtype=torch.int32, device=xyz.device)
    w3 = torch.zeros((B, N, 3), dtype=torch.float32, device=xyz.device)
    S = center.shape[1]
    ws, wsb = _workspace("cmdiad_interp3nn_workspace_bytes", xyz.device, B, S)      # the binned centres of the neighbourhood search (S >= 64)
    _call("cmdiad_interp3nn_ws", _p(xyz), _p(n_valid), _p(center), B, N, S, _p(idx3), _p(w3), _p(ws), wsb, _stream())
    return idx3, w3


def interp_gather(feat, idx3, w3, n_valid=None):
    """feat [B,S,D] f32 -> [B,N,D] f32 (pointnet2_utils.py:72)."""
    _chk(feat, torch.float32, "interp_gather.feat")
    B, S, D = feat.shape
    N = idx3.shape[1]
    out = torch.zeros((B, N, D), dtype=torch.float32, device=feat.device)
    _call("cmdiad_interp_gather", _p(feat), _p(idx3), _p(w3), _p(n_valid), B, N, S, D, _p(out), _stream())
    return out


def xyz_patch_fused(feat, idx3, w3, pix2pt, size=224, P=56, mean=0.0, inv_std=1.0, want_f32=True, want_bf16=False):
    """features.py:169-184 fused with the interpolation gather.  -> (patch_f32 [B,P*P,D] | None, bf16 | None)."""
    _chk(feat, torch.float32, "xyz_patch.feat")
    B, S, D = feat.shape
    N = idx3.shape[1]
    o32 = torch.empty((B, P * P, D), dtype=torch.float32, device=feat.device) if want_f32 else None
    o16 = torch.empty((B, P * P, D), dtype=torch.bfloat16, device=feat.device) if want_bf16 else None
    _call("cmdiad_xyz_patch_fused", _p(feat), _p(idx3), _p(w3), _p(pix2pt), B, N, S, D, size, P, float(mean),
          float(inv_std), _p(o32), _p(o16), _stream())
    return o32, o16


# ------------------------------------------------------------------------------------ dense blocks
def gemm(A, W, bias=None, act=ACT_NONE, residual=None, group_bias=None, group_rows=1, out_f32=None, out_bf16=None,
         want_f32=False, want_bf16=True, out_pre_bf16=None, dact_of=None, split_k=1, m_count=None,
         row_scale=None, ln_xb=None, ln_part=None, add2=None):
    """epilogue(A[M,K] . W[N,K]^T); A, W bf16.  Returns (out_f32 | None, out_bf16 | None).  m_count (device int32 [1]): only the
    first min(M, m_count) rows are computed and stored (a compacted row set whose size is known on the device only).
    LayerNorm fold (cmdiad_gemm_args, ABI 3): row_scale [>= M rounded up to 256] f32 multiplies the accumulator per row (consumer);
    ln_xb [M,N] bf16 + ln_part [N/64, M, 2] f32 (+ add2 [M,N] f32) are the producer's extra outputs of the in-place residual form."""
    _chk(A, torch.bfloat16, "gemm.A"); _chk(W, torch.bfloat16, "gemm.W")
    _chk(row_scale, torch.float32, "gemm.row_scale"); _chk(ln_xb, torch.bfloat16, "gemm.ln_xb")
    _chk(ln_part, torch.float32, "gemm.ln_part"); _chk(add2, torch.float32, "gemm.add2")
    M, K = A.shape
    N = W.shape[0]
    if row_scale is not None and row_scale.numel() < (M + 255) // 256 * 256:
        raise ValueError(f"gemm.row_scale: {row_scale.numel()} values, need M rounded up to 256 = {(M + 255) // 256 * 256}")
    if ln_part is not None and ln_part.numel() < (N // 64) * M * 2:
        raise ValueError(f"gemm.ln_part: {ln_part.numel()} values, need (N/64) * M * 2 = {(N // 64) * M * 2}")
    if out_f32 is None and want_f32:
        out_f32 = torch.empty((split_k, M, N) if split_k > 1 else (M, N), dtype=torch.float32, device=A.device)
    if out_bf16 is None and want_bf16:
        out_bf16 = torch.empty((M, N), dtype=torch.bfloat16, device=A.device)
    a = nat.GemmArgs(_p(A), K, _p(W), K, M, N, K, _p(bias), _p(group_bias), group_rows, act,
                     _p(residual), N, _p(out_f32), N, _p(out_bf16), N, _p(out_pre_bf16), _p(dact_of), split_k, _p(m_count),
                     _p(row_scale), _p(ln_xb), N, _p(ln_part), _p(add2), N)
    _call("cmdiad_gemm_bf16", ctypes.byref(a), _stream())
    return out_f32, out_bf16


_streamk_ws = {}


def gemm_streamk_eligible(M, N, K):
    return bool(nat.lib().cmdiad_gemm_streamk_eligible(M, N, K))


def gemm_streamk(A, W, bias, residual, out_f32=None):
    """out_f32 = A[M,K] . W[N,K]^T + bias + residual (in place when out_f32 is residual) on the stream-K kernel
    (cmdiad_gemm_streamk_bf16; bit-identical to gemm()).  The workspace (64 MiB of hand-over slots + counters, zeroed once) is kept
    per device; launches are serialised per device (see below)."""
    _chk(A, torch.bfloat16, "gemm_streamk.A"); _chk(W, torch.bfloat16, "gemm_streamk.W")
    _chk(bias, torch.float32, "gemm_streamk.bias"); _chk(residual, torch.float32, "gemm_streamk.residual")
    M, K = A.shape
    N = W.shape[0]
    if out_f32 is None:
        out_f32 = torch.empty((M, N), dtype=torch.float32, device=A.device)
    # ONE workspace and ONE launch in flight per device: block b of the kernel spins on block b - 1's counter, so two launches
    # that overlap (different streams) could fill every CU with waiting blocks whose predecessors are not resident yet -- a launch on
    # another stream first waits for the previous one's event
    key = A.device.index
    ent = _streamk_ws.get(key)
    if ent is None:
        ent = _streamk_ws[key] = {"ws": _workspace("cmdiad_gemm_streamk_workspace_bytes", A.device)[0].zero_(), "done": None,
                                  "stream": None}
    ws = ent["ws"]
    cur = torch.cuda.current_stream(A.device)
    # Not under stream capture: the cross-stream serialisation is an event recorded OUTSIDE the graph (waiting on it from inside a
    # capture, or keeping one that was recorded inside, invalidates the capture or raises), and replays of a captured stream-K
    # launch could overlap an eager one.  The plain tile kernel returns the same bits.
    if torch.cuda.is_current_stream_capturing():
        return gemm(A, W, bias=bias, residual=residual, out_f32=out_f32, want_f32=True, want_bf16=False)[0]
    if ent["done"] is not None and ent["stream"] != cur.cuda_stream:
        cur.wait_event(ent["done"])
    a = nat.GemmArgs(_p(A), K, _p(W), K, M, N, K, _p(bias), None, 1, ACT_NONE, _p(residual), N, _p(out_f32), N, None, 0, None, None, 1,
                     None, None, None, 0, None, None, 0)
    _call("cmdiad_gemm_streamk_bf16", ctypes.byref(a), _p(ws), ws.numel(), _stream())
    ent["done"] = torch.cuda.Event()
    ent["done"].record(cur)
    ent["stream"] = cur.cuda_stream
    return out_f32


def ln_stats_finalize(part, M, chunks, eps, rstd=None, want_mean=False):
    """part [chunks, M, 2] f32 (gemm(..., ln_part=)) -> rstd [M rounded up to 256] f32 (first M valid) (, mean [M])."""
    _chk(part, torch.float32, "ln_stats.part")
    if rstd is None:
        rstd = torch.empty(((M + 255) // 256 * 256,), dtype=torch.float32, device=part.device)
    mean = torch.empty((M,), dtype=torch.float32, device=part.device) if want_mean else None
    _call("cmdiad_ln_stats_finalize", _p(part), M, chunks, float(eps), _p(rstd), _p(mean), _stream())
    return (rstd, mean) if want_mean else rstd


def gemm_tn(P, Q, split_k=1, want_colsum=False):
    """sum_m P[m,:]^T Q[m,:]: P [M,N1], Q [M,N2] bf16 row-major -> f32 [N1,N2] (split_k == 1) or slabs [split_k,N1,N2];
    with want_colsum also the column sums of P ([N1] or [split_k,N1]) -> (out, colsum)."""
    _chk(P, torch.bfloat16, "gemm_tn.P"); _chk(Q, torch.bfloat16, "gemm_tn.Q")
    M, N1 = P.shape
    N2 = Q.shape[1]
    out = torch.empty((split_k, N1, N2) if split_k > 1 else (N1, N2), dtype=torch.float32, device=P.device)
    cs = torch.empty((split_k, N1) if split_k > 1 else (N1,), dtype=torch.float32, device=P.device) if want_colsum else None
    _call("cmdiad_gemm_tn_bf16", _p(P), N1, _p(Q), N2, M, N1, N2, split_k, _p(out), N2, _p(cs), _stream())
    return (out, cs) if want_colsum else out


def gemm_qkv(A, W, bias, B, T, q, k, vt, row_scale=None):
    """A [B*T,C] bf16 -> q,k [B,H,Tp,64], vt [B,H,64,Tp] (pre-allocated, zero-initialised padding).  row_scale [B*T] f32:
    the LayerNorm-folded form (qkv = row_scale[m] * (A . W^T) + bias)."""
    _chk(A, torch.bfloat16, "qkv.A"); _chk(W, torch.bfloat16, "qkv.W"); _chk(row_scale, torch.float32, "qkv.row_scale")
    C = A.shape[1]
    _call("cmdiad_gemm_qkv", _p(A), _p(W), _p(bias), _p(row_scale), B, T, C, _p(q), _p(k), _p(vt), _stream())


def attention(q, k, vt, B, H, T, out=None):
    """-> out [B*T, H*64] bf16."""
    if out is None:
        out = torch.empty((B * T, H * 64), dtype=torch.bfloat16, device=q.device)
    _call("cmdiad_attention", _p(q), _p(k), _p(vt), B, H, T, _p(out), _stream())
    return out


def encoder_tail(h2, gb, W3b, W4, b4, groups, Mg):
    """h2 [groups*Mg,256] bf16, gb [groups,512] f32 -> tokens [groups,384] f32 (h3 never leaves LDS): encoder_tail_n at
    Point-MAE's width."""
    if W4.shape[0] != 384:
        raise ValueError(f"tail: Point-MAE's W4 is [384, 512], got {tuple(W4.shape)}")
    return encoder_tail_n(h2, gb, W3b, W4, b4, groups, Mg)


def encoder_tail_n(h2, gb, W3b, W4, b4, groups, Mg, seg=0, out=None):
    """cmdiad_encoder_tail_n: tokens [groups, N] f32 at N = W4.shape[0] (256 or 384).  seg > 0 (N = 256): group g goes to row
    g + g // seg + 1 of out [groups + groups // seg, N], whose first row of every seg-group cloud is left unwritten."""
    _chk(h2, torch.bfloat16, "tail.h2"); _chk(gb, torch.float32, "tail.gb")
    N = W4.shape[0]
    if tuple(h2.shape) != (groups * Mg, 256) or tuple(gb.shape) != (groups, 512) or tuple(W4.shape) != (N, 512) or b4.numel() != N:
        raise ValueError(f"tail: h2 {tuple(h2.shape)}, gb {tuple(gb.shape)}, W4 {tuple(W4.shape)} for {groups} groups of {Mg}")
    rows = groups + (groups // seg if seg else 0)
    if out is None:
        out = torch.empty((rows, N), dtype=torch.float32, device=h2.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (rows, N):
        raise ValueError(f"tail.out: need a contiguous f32 [{rows}, {N}] tensor, got {out.dtype} {tuple(out.shape)}")
    _call("cmdiad_encoder_tail_n", _p(h2), _p(gb), _p(W3b), _p(W4), _p(b4), groups, Mg, N, seg, _p(out), _stream())
    return out


def conv2d_nhwc(x, W, N, ksize=3, stride=1, bias=None, act=ACT_NONE, residual=None, out_f32=None, out_bf16=None,
                want_f32=False, want_bf16=True):
    """x [B,H,W,C] bf16 NHWC, W [N, ksize*ksize*C] bf16 (tap-major) -> (out_f32 | None, out_bf16 | None), each [B,Ho,Wo,ld]
    with ld = the given buffer's last dimension (>= N; extra columns are left untouched).  cmdiad_conv2d_nhwc_bf16."""
    _chk(x, torch.bfloat16, "conv.x"); _chk(W, torch.bfloat16, "conv.W"); _chk(residual, torch.float32, "conv.residual")
    B, H, Wd, C = x.shape
    pad = 1 if ksize == 3 else 0
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (Wd + 2 * pad - ksize) // stride + 1
    if out_f32 is None and want_f32:
        out_f32 = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=x.device)
    if out_bf16 is None and want_bf16:
        out_bf16 = torch.empty((B, Ho, Wo, N), dtype=torch.bfloat16, device=x.device)
    a = nat.ConvArgs(_p(x), B, H, Wd, C, _p(W), N, ksize, stride, _p(bias), act,
                     _p(residual), residual.shape[-1] if residual is not None else 0,
                     _p(out_f32), out_f32.shape[-1] if out_f32 is not None else 0,
                     _p(out_bf16), out_bf16.shape[-1] if out_bf16 is not None else 0)
    _call("cmdiad_conv2d_nhwc_bf16", ctypes.byref(a), _stream())
    return out_f32, out_bf16


def im2col3x3(img, stride=2, ld=64):
    """img [B,C,H,W] f32 -> [B*Ho*Wo, ld] bf16, column c * 9 + ky * 3 + kx (padding 1; zero beyond 9 C): cmdiad_im2col3x3_bf16."""
    _chk(img, torch.float32, "im2col3x3.img")
    B, C, H, W = img.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    cols = torch.empty((B * Ho * Wo, ld), dtype=torch.bfloat16, device=img.device)
    _call("cmdiad_im2col3x3_bf16", _p(img), B, C, H, W, stride, ld, _p(cols), _stream())
    return cols


def conv_stem(x, w, bias, stride=2):
    """x [B,Cin<=4,H,W] f32 NCHW, w [Cout,Cin,3,3] f32 (BatchNorm folded), bias [Cout] -> ReLU(conv) as bf16 NHWC."""
    _chk(x, torch.float32, "stem.x"); _chk(w, torch.float32, "stem.w"); _chk(bias, torch.float32, "stem.bias")
    B, Cin, H, Wd = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
    out = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_conv_stem", _p(x), _p(w), _p(bias), B, Cin, H, Wd, Cout, stride, _p(out), _stream())
    return out


def upsample_bicubic(x, C, H, W, out_bf16=None, nchw=False):
    """x [B,h,w,ld] f32 NHWC (first C channels used) -> bf16 NHWC [B,H,W,ldo] (given or allocated with ldo = C) or, with
    nchw=True, f32 [B,C,H,W].  torch's bicubic, align_corners=False (cmdiad_upsample_bicubic)."""
    _chk(x, torch.float32, "bicubic.x")
    B, h, w, ld = x.shape
    if nchw:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        _call("cmdiad_upsample_bicubic", _p(x), B, h, w, C, ld, H, W, None, 0, _p(out), _stream())
        return out
    if out_bf16 is None:
        out_bf16 = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_upsample_bicubic", _p(x), B, h, w, C, ld, H, W, _p(out_bf16), out_bf16.shape[-1], None, _stream())
    return out_bf16


def transformer_block_workspace_bytes(M, C, hidden):
    return int(nat.lib().cmdiad_transformer_block_workspace_bytes(M, C, hidden))


BLOCK_LN1_READY, BLOCK_PREP_NEXT = 1, 2   # include/cmdiad_hip.h CMDIAD_BLOCK_*
_BLOCK_FIELDS = ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
                 "qkv_wf", "qkv_bf", "fc1_wf", "fc1_bf")


def transformer_block(x, pos, blk, B, T, H, eps, q, k, vt, workspace, flags=0):
    """x [B*T, C] f32 updated in place by one whole pre-LN block (cmdiad_transformer_block_fwd).  blk: dict of packed
    weights (runtime._pack_block); its ctypes struct is built once and cached in the dict.  flags: BLOCK_LN1_READY /
    BLOCK_PREP_NEXT chain the LayerNorm fold across consecutive calls on one workspace (needs blk's folded weights)."""
    _chk(x, torch.float32, "block.x"); _chk(pos, torch.float32, "block.pos")
    w = blk.get("_struct")
    if w is None:
        w = nat.BlockWeights(*[blk[n].data_ptr() if blk.get(n) is not None else None for n in _BLOCK_FIELDS])
        blk["_struct"] = w
    C = x.shape[1]
    _call("cmdiad_transformer_block_fwd", _p(x), _p(pos), ctypes.byref(w), B, T, C, H, blk["fc1_w"].shape[0], float(eps), int(flags),
          _p(q), _p(k), _p(vt), _p(workspace), workspace.numel(), _stream())
    return x


def layernorm(x, gamma, beta, eps, add=None, out_bf16=None, out_f32=None, want_bf16=True, stats=None):
    """x [M,C] f32 (updated in place to x+add when add is given) -> LN(x) as bf16 and/or f32."""
    _chk(x, torch.float32, "ln.x"); _chk(add, torch.float32, "ln.add")
    M, C = x.shape
    if out_bf16 is None and want_bf16:
        out_bf16 = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    ld = out_f32.stride(0) if out_f32 is not None else 0
    mean_o, rstd_o = stats if stats is not None else (None, None)
    _call("cmdiad_layernorm", _p(x), _p(add), _p(gamma), _p(beta), float(eps), M, C, _p(out_bf16), _p(out_f32), ld,
          _p(mean_o), _p(rstd_o), _stream())
    return out_bf16


def layernorm_skip_first(x, gamma, beta, eps, B, T, out_f32):
    """x [B*T, C] f32 -> LN of every row but the first of each T-row segment into out_f32 [B*(T-1), >= C] (a column slice is fine)."""
    _chk(x, torch.float32, "ln_skip.x")
    C = x.shape[1]
    if x.shape[0] != B * T or gamma.numel() != C or beta.numel() != C:
        raise ValueError(f"ln_skip: x {tuple(x.shape)} is not [{B} x {T}, C] or gamma / beta are not [C]")
    if out_f32.dtype != torch.float32 or out_f32.stride(1) != 1 or out_f32.shape[0] != B * (T - 1) or out_f32.shape[1] != C:
        raise ValueError(f"ln_skip.out_f32: need f32 [{B * (T - 1)}, {C}] with unit column stride")
    _call("cmdiad_layernorm_skip_first", _p(x), _p(gamma), _p(beta), float(eps), B, T, C, _p(out_f32), out_f32.stride(0), _stream())
    return out_f32


def lead_rows(x, pos, lead_x, lead_pos, B, T):
    """Row b*T of x (and of pos) <- lead_x (lead_pos), in place; x, pos [B*T, C] f32."""
    _chk(x, torch.float32, "lead.x"); _chk(pos, torch.float32, "lead.pos")
    C = x.shape[1]
    if x.shape[0] != B * T or (pos is not None and pos.shape != x.shape) or lead_x.numel() != C or (pos is not None and lead_pos.numel() != C):
        raise ValueError(f"lead: x {tuple(x.shape)} is not [{B} x {T}, C], or pos / the lead rows do not match it")
    _call("cmdiad_lead_rows", _p(x), _p(pos), _p(lead_x), _p(lead_pos), B, T, x.shape[1], _stream())
    return x


def col_sums(x):
    """x [rows, C] f32 -> [2, C] float64: the column sums of x and of x^2 (cmdiad_col_moments)."""
    _chk(x, torch.float32, "col_sums.x")
    rows, C = x.shape
    acc = torch.zeros((2, C), dtype=torch.float64, device=x.device)
    _call("cmdiad_col_moments", _p(x), rows, C, x.stride(0), _p(acc[0]), _p(acc[1]), _stream())
    return acc


def col_moments(x):
    """x [rows, C] f32 -> (mean [C], biased variance [C]) in float64 (cmdiad_col_moments)."""
    acc, rows = col_sums(x), x.shape[0]
    mean = acc[0] / rows
    return mean, acc[1] / rows - mean * mean


def bn_affine(sums, gamma, beta, rows, eps):
    """sums [2, C] f64 (col_sums of the rows-row batch), gamma, beta [C] f32 -> ((scale, shift, mean, rstd) f32, (mean, biased
    variance) f64): the constants of batch-statistics BatchNorm, y = z * scale + shift (cmdiad_bn_affine)."""
    _chk(sums, torch.float64, "bn_affine.sums"); _chk(gamma, torch.float32, "bn_affine.gamma"); _chk(beta, torch.float32, "bn_affine.beta")
    C = sums.shape[1]
    st64 = torch.empty((2, C), dtype=torch.float64, device=sums.device)
    aff = torch.empty((4, C), dtype=torch.float32, device=sums.device)
    _call("cmdiad_bn_affine", _p(sums[0]), _p(sums[1]), _p(gamma), _p(beta), rows, float(eps), C, _p(st64[0]), _p(st64[1]),
          _p(aff[0]), _p(aff[1]), _p(aff[2]), _p(aff[3]), _stream())
    return (aff[0], aff[1], aff[2], aff[3]), (st64[0], st64[1])


def bn_relu_fwd(z, scale, shift, residual=None, relu=True, want_bf16=True, want_f32=False):
    """z [M,C] f32 -> z * scale + shift (+ residual) (ReLU) as bf16 [M,C] (and / or f32): batch-statistics BatchNorm2d + ReLU
    (cmdiad_bn_relu_fwd).  Returns the bf16 tensor, or (bf16 | None, f32) when want_f32."""
    _chk(z, torch.float32, "bn_relu.z"); _chk(scale, torch.float32, "bn_relu.scale"); _chk(shift, torch.float32, "bn_relu.shift")
    _chk(residual, torch.float32, "bn_relu.residual")
    M, C = z.shape
    y = torch.empty((M, C), dtype=torch.bfloat16, device=z.device) if want_bf16 else None
    y32 = torch.empty((M, C), dtype=torch.float32, device=z.device) if want_f32 else None
    _call("cmdiad_bn_relu_fwd", _p(z), _p(scale), _p(shift), _p(residual), 1 if relu else 0, M, C, _p(y), _p(y32), _stream())
    return (y, y32) if want_f32 else y


def bn_relu_bwd(dy, z, scale, shift, mean, rstd, chunks=None, masked=True):
    """Backward of bn_relu_fwd: dy, z [M,C] f32; per-channel f32 vectors -> (dz bf16 [M,C], dgamma [C], dbeta [C]).  masked=False:
    the layer had no ReLU of its own (dy already carries the mask of the ReLU after the residual sum).
    (cmdiad_bn_relu_bwd_reduce -> cmdiad_bn_partials_sum -> cmdiad_bn_relu_bwd_apply)."""
    _chk(dy, torch.float32, "bn_bwd.dy"); _chk(z, torch.float32, "bn_bwd.z")
    M, C = z.shape
    if chunks is None:   # ~128 rows per workgroup (64 columns x 4 row lanes each), at most 256 row ranges
        chunks = max(16, min(256, (M + 127) // 128))
    mk = 1 if masked else 0
    p1 = torch.empty((chunks, C), dtype=torch.float32, device=z.device)
    p2 = torch.empty((chunks, C), dtype=torch.float32, device=z.device)
    _call("cmdiad_bn_relu_bwd_reduce", _p(dy), _p(z), _p(scale), _p(shift), _p(mean), _p(rstd), mk, M, C, chunks, _p(p1), _p(p2), _stream())
    dbeta = torch.empty((C,), dtype=torch.float32, device=z.device)
    dgamma = torch.empty((C,), dtype=torch.float32, device=z.device)
    _call("cmdiad_bn_partials_sum", _p(p1), _p(p2), chunks, C, _p(dbeta), _p(dgamma), _stream())
    dz = torch.empty((M, C), dtype=torch.bfloat16, device=z.device)
    _call("cmdiad_bn_relu_bwd_apply", _p(dy), _p(z), _p(scale), _p(shift), _p(mean), _p(rstd), _p(dbeta), _p(dgamma), mk, M, C, _p(dz),
          _stream())
    return dz, dgamma, dbeta


def loss_head(pred, target, mode, out_act, inv_b, want_grad=True, want_y=False):
    """pred, target [M,D] f32 -> (row_loss [M] f32, dpred [M,D] bf16 | None[, y [M,D] f32]): the LOSS_* row loss of
    y = LOSS_OUT_*(pred) against target, dpred = inv_b * d sum(row_loss) / d pred (cmdiad_loss_head)."""
    _chk(pred, torch.float32, "loss_head.pred"); _chk(target, torch.float32, "loss_head.target")
    M, D = pred.shape
    if tuple(target.shape) != (M, D):
        raise ValueError(f"loss_head: pred {tuple(pred.shape)} against target {tuple(target.shape)}")
    row_loss = torch.empty((M,), dtype=torch.float32, device=pred.device)
    dpred = torch.empty((M, D), dtype=torch.bfloat16, device=pred.device) if want_grad else None
    y = torch.empty((M, D), dtype=torch.float32, device=pred.device) if want_y else None
    _call("cmdiad_loss_head", _p(pred), _p(target), M, D, mode + out_act, inv_b, _p(row_loss), _p(dpred), _p(y), _stream())
    return (row_loss, dpred, y) if want_y else (row_loss, dpred)


def sum_vector(x, scale=1.0):
    """x [n] f32 -> scale * sum(x) as a 0-dim f32 tensor, in a fixed order (cmdiad_sum_vector)."""
    _chk(x, torch.float32, "sum_vector.x")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _call("cmdiad_sum_vector", _p(x), x.numel(), scale, _p(out), _stream())
    return out


def loss_and_grad(pred, target, mode, batch, need_grad, out_act=LOSS_OUT_NONE):
    """The tail of every training head: -> (loss 0-dim f32 = sum of the row losses / batch, dpred [M,D] bf16 = d loss / d pred |
    None).  loss_head + sum_vector, 1 / batch in both."""
    row_loss, dpred = loss_head(pred, target, mode, out_act, 1.0 / batch, want_grad=need_grad)
    return sum_vector(row_loss, 1.0 / batch), dpred


def reduce_slabs(slabs, S, n, out, scale=1.0):
    """out[:n] = scale * (slabs[0] + ... + slabs[S - 1]) in that order: slabs [S, n] f32 (any shape of n values per slab), out f32
    (cmdiad_reduce_slabs)."""
    _chk(slabs, torch.float32, "reduce_slabs.slabs"); _chk(out, torch.float32, "reduce_slabs.out")
    if slabs.numel() < S * n or out.numel() < n:
        raise ValueError(f"reduce_slabs: {S} slabs of {n} values from {slabs.numel()}, into {out.numel()}")
    _call("cmdiad_reduce_slabs", _p(slabs), S, n, n, float(scale), _p(out), _stream())
    return out


def colsum_bf16(x, chunks):
    """x [M,N] bf16 -> [chunks, N] f32: the column sums of each chunk of ceil(M / chunks) rows (cmdiad_colsum_bf16)."""
    _chk(x, torch.bfloat16, "colsum.x")
    M, N = x.shape
    part = torch.empty((chunks, N), dtype=torch.float32, device=x.device)
    _call("cmdiad_colsum_bf16", _p(x), M, N, chunks, _p(part), _stream())
    return part


def ln_param_grad(dh, x, mean, rstd, chunks):
    """dh, x [M,C] f32 (x: the LayerNorm's input), mean, rstd [M] f32 (its saved row statistics) -> the partial weight and bias
    gradients of each chunk of rows, two [chunks, C] f32 (cmdiad_ln_param_grad; reduce_slabs sums them)."""
    for t, n in ((dh, "dh"), (x, "x"), (mean, "mean"), (rstd, "rstd")):
        _chk(t, torch.float32, "ln_param_grad." + n)
    M, C = x.shape
    if tuple(dh.shape) != (M, C) or mean.numel() != M or rstd.numel() != M:
        raise ValueError(f"ln_param_grad: dh {tuple(dh.shape)}, x {tuple(x.shape)}, {mean.numel()} / {rstd.numel()} row statistics")
    pg = torch.empty((chunks, C), dtype=torch.float32, device=x.device)
    pb = torch.empty((chunks, C), dtype=torch.float32, device=x.device)
    _call("cmdiad_ln_param_grad", _p(dh), _p(x), _p(mean), _p(rstd), M, C, chunks, _p(pg), _p(pb), _stream())
    return pg, pb


def adam_step(p, grad, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, p_bf16=None):
    """torch.optim.Adam's update of p (no weight decay, no amsgrad) on grad * grad_scale, in place in p, m, v (f32, same size);
    p_bf16: refreshed with the bf16 cast of the new p (cmdiad_adam_step)."""
    for t, n in ((p, "p"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, torch.float32, "adam_step." + n)
    _chk(p_bf16, torch.bfloat16, "adam_step.p_bf16")
    if not grad.numel() == m.numel() == v.numel() == p.numel():
        raise ValueError("adam_step: p, grad, m and v must have the same number of elements")
    _call("cmdiad_adam_step", _p(p), _p(grad), _p(m), _p(v), p.numel(), float(lr), beta1, beta2, eps, step, float(grad_scale),
          _p(p_bf16), _stream())


def adam_flat(p, grad, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, p_bf16=None):
    """adam_step over a flat arena in ONE launch: p, grad, m, v f32 of the same size, a multiple of 4 elements, 16-byte aligned
    (dp_train.ParamArena's buffers).  Bit-identical to adam_step per parameter on equal inputs (cmdiad_adam_flat)."""
    for t, n in ((p, "p"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, torch.float32, "adam_flat." + n)
    _chk(p_bf16, torch.bfloat16, "adam_flat.p_bf16")
    if not grad.numel() == m.numel() == v.numel() == p.numel() or (p_bf16 is not None and p_bf16.numel() != p.numel()):
        raise ValueError("adam_flat: p, grad, m, v (and p_bf16) must have the same number of elements")
    _call("cmdiad_adam_flat", _p(p), _p(grad), _p(m), _p(v), p.numel(), float(lr), beta1, beta2, eps, int(step), float(grad_scale),
          _p(p_bf16), _stream())


def relu_bwd(dx, y, want_bf16=True, want_f32=False):
    """dx f32, y bf16 (the ReLU output), same shape -> dx where y > 0 else 0, as bf16 (and / or f32) (cmdiad_relu_bwd_bf16)."""
    _chk(dx, torch.float32, "relu_bwd.dx"); _chk(y, torch.bfloat16, "relu_bwd.y")
    assert dx.shape == y.shape
    dz = torch.empty(y.shape, dtype=torch.bfloat16, device=y.device) if want_bf16 else None
    dz32 = torch.empty(y.shape, dtype=torch.float32, device=y.device) if want_f32 else None
    _call("cmdiad_relu_bwd_bf16", _p(dx), _p(y), dx.numel(), _p(dz), _p(dz32), _stream())
    return (dz, dz32) if want_f32 else dz


def upsample_bicubic_bwd(grad_out, h, w):
    """grad_out [B,H,W,C] f32 NHWC -> gradient of the [B,h,w,C] input of upsample_bicubic (cmdiad_upsample_bicubic_bwd)."""
    _chk(grad_out, torch.float32, "bicubic_bwd.grad_out")
    B, H, W, C = grad_out.shape
    tmp = torch.empty((B, H, w, C), dtype=torch.float32, device=grad_out.device)
    out = torch.empty((B, h, w, C), dtype=torch.float32, device=grad_out.device)
    _call("cmdiad_upsample_bicubic_bwd", _p(grad_out), B, H, W, C, h, w, _p(tmp), _p(out), _stream())
    return out


def pad_nhwc(x, rows_multiple=64):
    """x [B,H,W,C] bf16 -> (buffer [guard + rows + guard, C] bf16, guard, rows): the zero-bordered copy [B,H+2,W+2,C] flattened to
    rows (zero-padded up to a multiple of rows_multiple), between two zero guards of W+3 rows so that every 3x3 tap's row
    offset stays inside the buffer (cmdiad_pad_nhwc_bf16)."""
    _chk(x, torch.bfloat16, "pad.x")
    B, H, W, C = x.shape
    guard = W + 3
    rows = (B * (H + 2) * (W + 2) + rows_multiple - 1) // rows_multiple * rows_multiple
    buf = torch.zeros((guard + rows + guard, C), dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_pad_nhwc_bf16", _p(x), B, H, W, C, _p(buf[guard:]), _stream())
    return buf, guard, rows


def moments3(xyz):
    """xyz [rows, 3] f32 -> (mean [3], covariance [3,3]) in float64, biased (cmdiad_moments3)."""
    _chk(xyz, torch.float32, "moments3.xyz")
    rows = xyz.shape[0]
    acc = torch.zeros((9,), dtype=torch.float64, device=xyz.device)
    _call("cmdiad_moments3", _p(xyz), rows, _p(acc), _stream())
    mean = acc[:3] / rows
    m2 = torch.stack([acc[[3, 4, 5]], acc[[4, 6, 7]], acc[[5, 7, 8]]]) / rows
    return mean, m2 - torch.outer(mean, mean)


def encoder_stage1(neigh, w1b1, W2, b2, groups, Mg):
    """-> (h2 [groups*Mg,256] bf16, gmax [groups,256] f32, gmax_bf16)."""
    dev = neigh.device
    h2 = torch.empty((groups * Mg, 256), dtype=torch.bfloat16, device=dev)
    g32 = torch.empty((groups, 256), dtype=torch.float32, device=dev)
    g16 = torch.empty((groups, 256), dtype=torch.bfloat16, device=dev)
    _call("cmdiad_encoder_stage1", _p(neigh), _p(w1b1), _p(W2), _p(b2), groups, Mg, _p(h2), _p(g32), _p(g16), _stream())
    return h2, g32, g16


def gemm_groupmax(A, W, bias, groups, Mg, want_bf16=False):
    N, K = W.shape
    o32 = torch.empty((groups, N), dtype=torch.float32, device=A.device)
    o16 = torch.empty((groups, N), dtype=torch.bfloat16, device=A.device) if want_bf16 else None
    _call("cmdiad_gemm_groupmax", _p(A), _p(W), _p(bias), groups, Mg, N, K, _p(o32), _p(o16), _stream())
    return o32, o16


# ------------------------------------------------------------------------------------ scoring
# 16-bit operand type of the patch-library distance GEMM.  bfloat16 since round 5: the same kernel runs 6.5 % faster on bf16 operands
# than on fp16 ones (5.05-5.16 against 5.38-5.57 ms, same box: fewer mantissa bits toggle, the chip holds a higher clock --
# profiles/r5_notes.md section 6), and what the three mantissa bits buy is invisible behind the extractor's own 16-bit noise: the
# operand rounding moves a distance of 4-35 by ~0.03, the bf16 feature chain by ~0.5 (tests/test_gpu_predictor.py: image scores,
# pixel maps and AUROCs identical to the last printed digit on both types); the winner is re-scored in fp32 either way.
# CMDIAD_SEARCH_DTYPE=fp16 restores IEEE half operands.
SEARCH_DTYPE = torch.float16 if os.environ.get("CMDIAD_SEARCH_DTYPE", "bf16").lower() in ("fp16", "float16", "half") else torch.bfloat16


def normalize_cast(x, mean=0.0, inv_std=1.0, want_f32=False, want_sq=True, dtype=None, skip_leading=0):
    """x [rows,D] f32 -> (16-bit [rows,D] (the search operand type: bf16 by default, or fp16), f32 normalised | None,
    row |.|^2 of the ROUNDED rows | None).
    skip_leading = s > 0: x is [G, s + R, D] and the first s rows of every group are not taken (the cls token of the ViT's
    [B, 785, C] tokens): outputs have G * R rows, read in place -- no gather copy of the patch rows in between."""
    _chk(x, torch.float32, "normalize_cast.x")
    dtype = dtype or SEARCH_DTYPE
    if skip_leading:
        G, T, D = x.shape
        group = T - skip_leading
        rows = G * group
    else:
        rows, D = x.shape
        group = 0
    o16 = torch.empty((rows, D), dtype=dtype, device=x.device)
    o32 = torch.empty((rows, D), dtype=torch.float32, device=x.device) if want_f32 else None
    sq = torch.empty((rows,), dtype=torch.float32, device=x.device) if want_sq else None
    _call("cmdiad_normalize_cast_rows", _p(x), rows, D, group, int(skip_leading), float(mean), float(inv_std), _p(o16), _p(o32), _p(sq),
          1 if dtype == torch.float16 else 0, _stream())
    return o16, o32, sq


def new_keys(Q, device, runner=False):
    """Packed nearest-neighbour keys, "no candidate" everywhere.  runner=True: [2, Q] -- plane 0 the best row of every query,
    plane 1 its runner-up (the nearest row outside the winner's group of 16 rows, include/cmdiad_hip.h) for the exact fp32
    decision of l2_rescore; every function below that takes `keys` accepts either shape."""
    return torch.full((2, Q) if runner else (Q,), KEY_EMPTY, dtype=torch.int64, device=device)


def _key_planes(keys, n, name):
    """-> (pointer of the best plane, pointer of the runner-up plane or None) of a [n] or [2, n] int64 key tensor."""
    _chk(keys, torch.int64, name)
    if keys.dim() == 2:
        if keys.shape[0] != 2 or keys.shape[1] < n:
            raise ValueError(f"{name}: expected [2, >={n}] keys, got {tuple(keys.shape)}")
        return _p(keys[0]), _p(keys[1])
    if keys.shape[0] < n:
        raise ValueError(f"{name}: {keys.shape[0]} keys for {n} query rows")
    return _p(keys), None


def l2_min_keys(q16, q_sq, bank16, bank_sq, keys, row_offset=0):
    Q, D = q16.shape
    if q16.dtype != bank16.dtype:
        raise TypeError("l2_min_keys: queries and bank must share the 16-bit dtype")
    k1, k2 = _key_planes(keys, Q, "l2_min_keys.keys")
    _call("cmdiad_l2_min_keys", _p(q16), _p(q_sq), _p(bank16), _p(bank_sq), Q, bank16.shape[0], D, row_offset,
          k1, k2, 1 if q16.dtype == torch.float16 else 0, _stream())
    return keys


class DedupPlan:
    """Device-resident plan of cmdiad_rows_dedup_plan: slot [Q] i32 (compacted row answering for q), rows [Q] i32, count [1] i32,
    q16 [Q,D] / q_sq [Q] (first count rows live).  Buffers are reused when one is passed back in."""
    __slots__ = ("slot", "rows", "count", "q16", "q_sq", "work")

    def __init__(self, Q, D, dtype, device):
        self.slot = torch.empty((Q,), dtype=torch.int32, device=device)
        self.rows = torch.empty((Q,), dtype=torch.int32, device=device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=device)
        self.q16 = torch.empty((Q, D), dtype=dtype, device=device)
        self.q_sq = torch.empty((Q,), dtype=torch.float32, device=device)
        self.work = _workspace("cmdiad_rows_dedup_workspace_bytes", device, Q)[0]


def rows_dedup_plan(q16, q_sq, plan=None):
    """Exact removal of the repeated constant rows (patches without a foreground pixel) of a 16-bit query set: include/cmdiad_hip.h."""
    Q, D = q16.shape
    if q16.dtype not in (torch.float16, torch.bfloat16) or not q16.is_contiguous():
        raise TypeError("rows_dedup_plan: contiguous 16-bit queries")
    _chk(q_sq, torch.float32, "rows_dedup_plan.q_sq")
    if plan is None or plan.q16.shape != q16.shape or plan.q16.dtype != q16.dtype:
        plan = DedupPlan(Q, D, q16.dtype, q16.device)
    # a 0-row tensor has no address and the entry point wants non-null pointers: at Q = 0 it reads and writes none of them but count
    p = (lambda t: _p(plan.work)) if Q == 0 else _p
    _call("cmdiad_rows_dedup_plan", p(q16), p(q_sq), Q, D, _p(plan.work), p(plan.slot), p(plan.rows), _p(plan.count),
          p(plan.q16), p(plan.q_sq), _stream())
    return plan


def l2_min_keys_counted(q16, q_sq, count, bank16, bank_sq, keys, row_offset=0):
    """l2_min_keys over the first count[0] (device int32) rows of q16."""
    Q, D = q16.shape
    if q16.dtype != bank16.dtype:
        raise TypeError("l2_min_keys_counted: queries and bank must share the 16-bit dtype")
    _chk(count, torch.int32, "l2_min_keys_counted.count")
    k1, k2 = _key_planes(keys, Q, "l2_min_keys_counted.keys")
    _call("cmdiad_l2_min_keys_counted", _p(q16), _p(q_sq), _p(count), Q, _p(bank16), _p(bank_sq), bank16.shape[0], D, row_offset,
          k1, k2, 1 if q16.dtype == torch.float16 else 0, _stream())
    return keys


def l2_min_keys_segments(q16, q_sq, seg_counts, seg_stride, bank16, bank_sq, keys, row_offset=0):
    """l2_min_keys over the segments [w * seg_stride, w * seg_stride + seg_counts[w]) of q16 (seg_counts: device int32 [n_seg]):
    ONE launch over the live query tiles of all segments (include/cmdiad_hip.h)."""
    Q, D = q16.shape
    if q16.dtype != bank16.dtype:
        raise TypeError("l2_min_keys_segments: queries and bank must share the 16-bit dtype")
    _chk(seg_counts, torch.int32, "l2_min_keys_segments.seg_counts")
    n_seg = seg_counts.shape[0]
    if n_seg * seg_stride != Q or keys.shape[-1] < Q:
        raise ValueError(f"l2_min_keys_segments: {n_seg} segments of {seg_stride} rows != {Q} query rows (keys: {keys.shape[-1]})")
    k1, k2 = _key_planes(keys, Q, "l2_min_keys_segments.keys")
    _call("cmdiad_l2_min_keys_segments", _p(q16), _p(q_sq), _p(seg_counts), n_seg, seg_stride, _p(bank16), _p(bank_sq),
          bank16.shape[0], D, row_offset, k1, k2, 1 if q16.dtype == torch.float16 else 0, _stream())
    return keys


def rows_expand_f32(rows_compact, slot, out=None):
    """out[q] = rows_compact[slot[q]] (f32 rows): per-row results computed on the compacted rows, back on every original row."""
    _chk(rows_compact, torch.float32, "rows_expand.rows"); _chk(slot, torch.int32, "rows_expand.slot")
    Q, D = slot.shape[0], rows_compact.shape[1]
    if out is None:
        out = torch.empty((Q, D), dtype=torch.float32, device=rows_compact.device)
    _call("cmdiad_rows_expand_f32", _p(rows_compact), _p(slot), Q, D, _p(out), _stream())
    return out


def keys_expand(keys_compact, slot, keys):
    """keys[..., q] = keys_compact[..., slot[q]] ([n] or [2, n] key tensors: both planes)."""
    _chk(slot, torch.int32, "keys_expand.slot")
    if keys_compact.dim() != keys.dim():
        raise ValueError("keys_expand: compact and expanded keys must have the same number of planes")
    if keys.dim() == 2:
        for pl in range(2):
            _call("cmdiad_keys_expand", _p(keys_compact[pl]), _p(slot), slot.shape[0], _p(keys[pl]), _stream())
        return keys
    _call("cmdiad_keys_expand", _p(keys_compact), _p(slot), slot.shape[0], _p(keys), _stream())
    return keys


def l2_rescore(q32, bank32, keys, min_val=None, min_idx=None, row_offset=0):
    """Exact fp32 distance and row of every query's nearest library row.  keys [Q]: the search's winner is taken as it is;
    keys [2, Q] (best + runner-up): both are measured in fp32 and the nearer one wins (ties: the lower row) -- torch.min on the
    fp32 distance matrix (features.py:227)."""
    Q, D = q32.shape
    if min_val is None:
        min_val = torch.zeros((Q,), dtype=torch.float32, device=q32.device)
        min_idx = torch.zeros((Q,), dtype=torch.int64, device=q32.device)
    if keys.dim() == 2:
        _call("cmdiad_l2_rescore2", _p(q32), _p(bank32), _p(keys[0]), _p(keys[1]), Q, bank32.shape[0], D, row_offset, None,
              _p(min_val), _p(min_idx), _stream())
        return min_val, min_idx
    _call("cmdiad_l2_rescore", _p(q32), _p(bank32), _p(keys), Q, bank32.shape[0], D, row_offset, _p(min_val),
          _p(min_idx), _stream())
    return min_val, min_idx


def l2_rescore_pair_d2(q32, bank32, keys, d2_pair, row_offset=0):
    """Squared fp32 distances [2, Q] of the candidates of keys [2, Q] whose rows lie in this shard's [row_offset, +rows); the other
    entries are left as they are (zero-filled by the caller, summed over the shards, then l2_choose)."""
    Q, D = q32.shape
    _call("cmdiad_l2_rescore2", _p(q32), _p(bank32), _p(keys[0]), _p(keys[1]), Q, bank32.shape[0], D, row_offset, _p(d2_pair),
          None, None, _stream())
    return d2_pair


def l2_choose(keys, d2_pair, min_val, min_idx):
    """The decision of l2_rescore on [2, Q] keys from squared distances that were summed over the shards."""
    _call("cmdiad_l2_choose", _p(keys[0]), _p(keys[1]), _p(d2_pair), keys.shape[1], _p(min_val), _p(min_idx), _stream())
    return min_val, min_idx


def score_head(min_val, min_idx, patch32, bank32, m_star, row_offset=0, rows=None):
    """features.py:227-235 per image.  min_val / min_idx [B*Q], patch32 [B,Q,D], bank32 = the rows [row_offset, row_offset + rows)
    of the library (rows: bank32.shape[0] unless given) -> (s_star [B], s_idx [B] i32, m_test [B,D]).  m_star [B,D] is the CALLER's
    prefilled buffer: row b is written only when the winning patch's library row lies in that window (its owner shard)."""
    B, Q, D = patch32.shape
    for t, n in ((min_val, "min_val"), (patch32, "patch"), (bank32, "bank"), (m_star, "m_star")):
        _chk(t, torch.float32, "score_head." + n)
    _chk(min_idx, torch.int64, "score_head.min_idx")
    dev = patch32.device
    s_star = torch.empty((B,), dtype=torch.float32, device=dev)
    s_idx = torch.empty((B,), dtype=torch.int32, device=dev)
    m_test = torch.empty((B, D), dtype=torch.float32, device=dev)
    _call("cmdiad_score_head", _p(min_val), _p(min_idx), _p(patch32), _p(bank32), B, Q, D, bank32.shape[0] if rows is None else rows,
          row_offset, _p(s_star), _p(s_idx), _p(m_test), _p(m_star), _stream())
    return s_star, s_idx, m_test


def score_tail(s_star, m_test, top3, bank32, knn_d, row_offset=0, rows=None):
    """features.py:285 per image: knn_d[b, k - 1] = || m_test[b] - row(top3[b, k]) ||, k = 1, 2.  knn_d [B,2] is the CALLER's
    prefilled buffer: an entry is written only when that row lies in [row_offset, row_offset + rows) (KEY_EMPTY names none)."""
    B, D = m_test.shape
    for t, n in ((s_star, "s_star"), (m_test, "m_test"), (bank32, "bank"), (knn_d, "knn_d")):
        _chk(t, torch.float32, "score_tail." + n)
    _chk(top3, torch.int64, "score_tail.top3")
    _call("cmdiad_score_tail", _p(s_star), _p(m_test), _p(top3), _p(bank32), B, D, bank32.shape[0] if rows is None else rows,
          row_offset, _p(knn_d), _stream())
    return knn_d


def score_final(s_star, knn_d, D):
    """features.py:286-290: s [B] = (1 - exp(s* / sqrt(D)) / (exp(knn_0 / sqrt(D)) + exp(knn_1 / sqrt(D)))) * s*."""
    _chk(s_star, torch.float32, "score_final.s_star"); _chk(knn_d, torch.float32, "score_final.knn_d")
    B = s_star.shape[0]
    s = torch.empty((B,), dtype=torch.float32, device=s_star.device)
    _call("cmdiad_score_final", _p(s_star), _p(knn_d), B, D, _p(s), _stream())
    return s


def bank_block16(bank32):
    """[Nb,D] f32 -> the library copy laid out for the fp32 matrix cores (cmdiad_bank_block16), a flat f32 tensor."""
    _chk(bank32, torch.float32, "bank_block16.bank")
    Nb, D = bank32.shape
    out = torch.empty((int(nat.lib().cmdiad_bank_block16_floats(Nb, D)),), dtype=torch.float32, device=bank32.device)
    _call("cmdiad_bank_block16", _p(bank32), Nb, D, _p(out), _stream())
    return out


def reweight_scan(probes, bank32, blk16=None, top3=None, row_offset=0):
    """probes [R,D] f32 -> top3 [R,3] packed keys (int64 view of u64; exact fp32 d2).  One pass over the library per 32
    probes.  blk16: ops.bank_block16(bank32) (built on the fly when absent -- engine.Bank keeps one)."""
    _chk(probes, torch.float32, "reweight.probes"); _chk(bank32, torch.float32, "reweight.bank")
    R, D = probes.shape
    Nb = bank32.shape[0]
    if blk16 is None:
        blk16 = bank_block16(bank32)
    if top3 is None:
        top3 = torch.full((R, 3), KEY_EMPTY, dtype=torch.int64, device=probes.device)
    for lo in range(0, R, 32):
        r = min(32, R - lo)
        ws, wsb = _workspace("cmdiad_reweight_workspace_bytes", probes.device, r, Nb)
        _call("cmdiad_reweight_scan", _p(probes[lo:lo + r]), _p(bank32), _p(blk16), r, Nb, D, row_offset, _p(top3[lo:lo + r]),
              _p(ws), wsb, _stream())
    return top3


def reweight_scan_pair(probes0, bank0, blk0, probes1, bank1, blk1, row_offset0=0, row_offset1=0):
    """reweight_scan for the TWO libraries of a scored batch in one launch pair (cmdiad_reweight_scan_pair): -> (top3_0, top3_1),
    each [R,3] packed keys, identical to two separate reweight_scan calls.  R <= 32 per library (a batch of 32 images)."""
    for t, n in ((probes0, "probes0"), (bank0, "bank0"), (probes1, "probes1"), (bank1, "bank1")):
        _chk(t, torch.float32, "reweight_pair." + n)
    (R0, D), R1 = probes0.shape, probes1.shape[0]
    Nb0, Nb1 = bank0.shape[0], bank1.shape[0]
    if R0 > 32 or R1 > 32 or Nb0 == 0 or Nb1 == 0 or probes1.shape[1] != D:
        raise ValueError("reweight_scan_pair: R <= 32 per library, both libraries non-empty, equal D")
    dev = probes0.device
    top0 = torch.full((R0, 3), KEY_EMPTY, dtype=torch.int64, device=dev)
    top1 = torch.full((R1, 3), KEY_EMPTY, dtype=torch.int64, device=dev)
    ws, wsb = _workspace("cmdiad_reweight_pair_workspace_bytes", dev, Nb0, Nb1)
    _call("cmdiad_reweight_scan_pair", _p(probes0), _p(bank0), _p(blk0), R0, Nb0, row_offset0, _p(top0),
          _p(probes1), _p(bank1), _p(blk1), R1, Nb1, row_offset1, _p(top1), D, _p(ws), wsb, _stream())
    return top0, top1


def l2_dist_matrix(q32, bank32):
    """Exact fp32 [Q,Nb] matrix of L2 distances (features.py:186-190 materialised; API compatibility only)."""
    _chk(q32, torch.float32, "dist_matrix.q"); _chk(bank32, torch.float32, "dist_matrix.bank")
    Q, D = q32.shape
    out = torch.empty((Q, bank32.shape[0]), dtype=torch.float32, device=q32.device)
    _call("cmdiad_l2_dist_matrix", _p(q32), _p(bank32), Q, bank32.shape[0], D, _p(out), _stream())
    return out


def unpack_keys(keys):
    """int64 view of packed u64 keys -> (value f32, index int64)."""
    idx = keys & 0xFFFFFFFF
    val = (keys >> 32).to(torch.int32).view(torch.float32) if keys.numel() else keys.float()
    return val, idx


# ------------------------------------------------------------------------------------ small ops
def im2col_patch8(rgb):
    _chk(rgb, torch.float32, "im2col.rgb")
    B, _, S, _ = rgb.shape
    out = torch.empty((B * (S // 8) ** 2, 192), dtype=torch.bfloat16, device=rgb.device)
    _call("cmdiad_im2col_patch8", _p(rgb), B, S, _p(out), _stream())
    return out


def im2col_patch14(rgb):
    """rgb [B,3,S,S] f32, S % 14 == 0 -> DINOv2's patch operand [B*(S/14)^2, 640] bf16: column c*196 + dy*14 + dx, 588.. zero."""
    _chk(rgb, torch.float32, "im2col14.rgb")
    B, _, S, _ = rgb.shape
    out = torch.empty((B * (S // 14) ** 2, 640), dtype=torch.bfloat16, device=rgb.device)
    _call("cmdiad_im2col_patch14", _p(rgb), B, S, _p(out), _stream())
    return out


def token_pool56(tokens):
    """tokens [B, 1 + s*s, C] f32 (cls row first) -> AdaptiveAvgPool2d((56, 56)) of the s x s patch grid, [B, 3136, C] f32, read in
    place (cmdiad_token_pool56: the bits of torch's CPU adaptive_avg_pool2d)."""
    _chk(tokens, torch.float32, "token_pool56.tokens")
    B, T, C = tokens.shape
    s = math.isqrt(T - 1)
    if s * s != T - 1:
        raise ValueError(f"token_pool56: {T - 1} patch tokens are not a square grid")
    out = torch.empty((B, 56 * 56, C), dtype=torch.float32, device=tokens.device)
    _call("cmdiad_token_pool56", _p(tokens), B, s, C, _p(out), _stream())
    return out


def vit_assemble(patch_out, cls, pos, B, P, C):
    tokens = torch.empty((B * (P + 1), C), dtype=torch.float32, device=patch_out.device)
    _call("cmdiad_vit_assemble", _p(patch_out), _p(cls), _p(pos), B, P, C, _p(tokens), _stream())
    return tokens


def bilinear_up(x, H):
    _chk(x, torch.float32, "bilinear.x")
    B, h, _ = x.shape
    out = torch.empty((B, H, H), dtype=torch.float32, device=x.device)
    _call("cmdiad_bilinear_up", _p(x), B, h, H, _p(out), _stream())
    return out


def blur8_maps(maps, radius=4.0):
    """KNNGaussianBlur (utils/utils.py:71-83) on device: maps [n,H,W] f32 -> [n,H,W] f32, bit-exact with Pillow's 8-bit path."""
    _chk(maps, torch.float32, "blur8.maps")
    n, H, W = maps.shape
    out = torch.empty_like(maps)
    _call("cmdiad_blur8_maps", _p(maps), n, H, W, float(radius), _p(out), _stream())
    return out


def ocsvm_score_maps(maps, lambdas, coef, offset):
    """seg_fuser.score_samples over the lambda-weighted map stack: maps [B,K,HW] f32 -> [B,HW] f64
    (multiple_features.py:985-992; coef / offset from a host-fitted sklearn SGDOneClassSVM)."""
    import ctypes
    import numpy as np
    _chk(maps, torch.float32, "ocsvm.maps")
    B, K, HW = maps.shape
    lam = np.ascontiguousarray(lambdas, dtype=np.float32)
    cf = np.ascontiguousarray(np.asarray(coef).reshape(-1), dtype=np.float64)
    assert lam.shape == (K,) and cf.shape == (K,)
    out = torch.empty((B, HW), dtype=torch.float64, device=maps.device)
    _call("cmdiad_ocsvm_score_maps", _p(maps), B, K, HW, lam.ctypes.data_as(ctypes.c_void_p), cf.ctypes.data_as(ctypes.c_void_p),
          float(np.asarray(offset).reshape(-1)[0]), _p(out), _stream())
    return out


def linear3(x, wb, act=ACT_NONE):
    """x [M,3] f32, wb [N,4] f32 -> act(W x + b) as bf16 [M,N]."""
    _chk(x, torch.float32, "linear3.x")
    M, N = x.shape[0], wb.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_linear3", _p(x), _p(wb), M, N, act, _p(out), _stream())
    return out


def cast_bf16(x):
    _chk(x, torch.float32, "cast.x")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_cast_bf16", _p(x), x.numel(), _p(out), _stream())
    return out


def transpose_bf16(x):
    _chk(x, torch.bfloat16, "transpose.x")
    r, c = x.shape
    out = torch.empty((c, r), dtype=torch.bfloat16, device=x.device)
    _call("cmdiad_transpose_bf16", _p(x), r, c, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------ frames: the limits and checks of the map ops
# csrc/frames.h's limits of a batch of n frames of H x W (tests/test_frame_limits_cpu.py holds the two together), and mesh.hip's total
FRAME_MAX_IMAGES, FRAME_MAX_PIXELS, FRAME_MAX_TOTAL, FRAME_MAX_SIDE = 65535, 1 << 24, 1 << 30, 1 << 14
MESH_MAX_TOTAL = 1 << 24
METRICS_MAX_TOTAL = ORGANIZE_MAX_TOTAL = FRAME_MAX_TOTAL
ORGANIZE_MAX_IMAGES, ORGANIZE_MAX_PIXELS, OVERLAY_MAX_SIDE = FRAME_MAX_IMAGES, FRAME_MAX_PIXELS, FRAME_MAX_SIDE


def _frames(shape, who, side=None, pixels=FRAME_MAX_PIXELS, total=FRAME_MAX_TOTAL, least=1, msg=None):
    """(n, H, W) of `shape` after THE frame-limit check: frames.h's sizes_ok by default.  side / pixels / total: the op's limit on a
    side, on H W and on n H W (None: no limit); least: the smallest side; msg: the refusal's text where the op has its own."""
    n, H, W = (int(v) for v in shape)
    limits = ((n, FRAME_MAX_IMAGES), (max(H, W), side), (H * W, pixels), (n * H * W, total))
    if min(H, W) < least or any(cap is not None and v > cap for v, cap in limits):
        raise ValueError(msg or f"{who}: unsupported shape {tuple(shape)} (n <= {FRAME_MAX_IMAGES}, H, W >= 1, H*W <= 2^24, n*H*W <= 2^30)")
    return n, H, W


def _chk_maps(maps, who, what="maps", dtype=torch.float64):
    _chk(maps, dtype, f"{who}.{what}")
    if maps.dim() != 3:
        raise ValueError(f"{who}: {what} must be [n,H,W], got {tuple(maps.shape)}")
    return _frames(maps.shape, who)


def _on_device(dev, who, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise ValueError(f"{who}.{name}: must be on {dev}, got {t.device}")


def _chk_out(t, dtype, shape, dev, name):
    _chk(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError(f"{name}: must be {tuple(shape)} {dtype} on {dev}, got {tuple(t.shape)} on {t.device}")


def _out(t, dtype, shape, dev, name, zero=False):
    """the caller's buffer after _chk_out, or a fresh one"""
    if t is None:
        return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=dev)
    _chk_out(t, dtype, shape, dev, name)
    return t


def _chk_region_tables(count, ints, n, who):
    """count [n] i32 and ints [n,K,8] i32, region_table's -> K"""
    _chk(count, torch.int32, f"{who}.count"); _chk(ints, torch.int32, f"{who}.ints")
    if count.numel() != n or ints.dim() != 3 or ints.shape[0] != n or ints.shape[2] != 8 or not 1 <= ints.shape[1] <= REGION_MAX:
        raise ValueError(f"{who}: count must be [{n}] and ints [{n},K,8] with K in 1..{REGION_MAX}; got {tuple(count.shape)}, "
                         f"{tuple(ints.shape)}")
    return ints.shape[1]


def _chk_colours(who, n, H, W, lohi, lut, alpha, background, mean, std):
    """the colour arguments overlay_render and mesh_write share, for an output of H x W -> (background kind, 1 where lohi is per
    image, mean, std as floats)"""
    _chk(lohi, torch.float64, f"{who}.lohi"); _chk(lut, torch.uint8, f"{who}.lut"); _chk(alpha, torch.uint8, f"{who}.alpha")
    if lohi is None or lut is None or alpha is None:
        raise ValueError(f"{who}: lohi, lut and alpha are required")
    if tuple(lohi.shape) not in ((2,), (1, 2), (n, 2)) or tuple(lut.shape) != (256, 3) or tuple(alpha.shape) != (256,):
        raise ValueError(f"{who}: lohi must be [2] or [{n},2], lut [256,3], alpha [256]; got {tuple(lohi.shape)}, "
                         f"{tuple(lut.shape)}, {tuple(alpha.shape)}")
    kind = 0
    if background is not None:
        if background.dtype not in OVERLAY_BACKGROUNDS[1:]:
            raise TypeError(f"{who}.background: expected uint8 [n,{H},{W},3] or float32 [n,3,{H},{W}], got {background.dtype}")
        kind = OVERLAY_BACKGROUNDS.index(background.dtype)
        _chk(background, background.dtype, f"{who}.background")
        want = (n, H, W, 3) if kind == 1 else (n, 3, H, W)
        if tuple(background.shape) != want:
            raise ValueError(f"{who}: a {background.dtype} background must be {want} (the output's size: it is not resampled), "
                             f"got {tuple(background.shape)}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"{who}: mean and std are three values each")
    return kind, int(lohi.numel() == 2 * n and n > 1), mean, std


# ------------------------------------------------------------------------------------ scan preprocessing (docs/preprocessing.md)
def plane_ransac(points, n=50, iterations=1000, distance_threshold=0.004, seed=0):
    """points [E,3] f32 -> (plane [4] f64 = (a, b, c, d) with unit normal and c >= 0, info [2] int32 = {inliers, winning hypothesis}),
    both on the device.  get_plane_eq of utils/preprocessing.py:30-33 under this project's RANSAC contract."""
    _chk(points, torch.float32, "plane_ransac.points")
    E = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"plane_ransac: points must be [E,3], got {tuple(points.shape)}")
    if E < n:
        raise ValueError(f"plane_ransac: {E} points, {n} needed for one sample")
    plane = torch.empty(4, dtype=torch.float64, device=points.device)
    info = torch.empty(2, dtype=torch.int32, device=points.device)
    ws, wsb = _workspace("cmdiad_plane_ransac_workspace_bytes", points.device, int(iterations))
    _call("cmdiad_plane_ransac", _p(points), E, int(n), int(iterations), float(distance_threshold), int(seed) & 0xFFFFFFFF,
          _p(plane), _p(info), _p(ws), wsb, _stream())
    return plane, info


def plane_mask(pc, rgb, plane, distance_threshold=0.005):
    """In place: pc [...,3] f32 and rgb [..., C] (any dtype, None = xyz only) are zeroed where the point is closer to `plane`
    ([4] f64 on the device) than distance_threshold (strict).  utils/preprocessing.py:46-50."""
    _chk(pc, torch.float32, "plane_mask.pc"); _chk(plane, torch.float64, "plane_mask.plane")
    n = pc.numel() // 3
    rgb_bytes = 0
    if rgb is not None:
        if not rgb.is_cuda:
            raise nat.NativeError("plane_mask.rgb: tensor must live on the GPU (cmdiad_amd has no CPU path)")
        if not rgb.is_contiguous():
            raise ValueError("plane_mask.rgb: tensor must be contiguous")
        if n == 0 or (rgb.numel() * rgb.element_size()) % n or rgb.numel() // n * n != rgb.numel():
            raise ValueError(f"plane_mask: rgb {tuple(rgb.shape)} does not match pc {tuple(pc.shape)}")
        rgb_bytes = rgb.numel() * rgb.element_size() // n
    _call("cmdiad_plane_mask", _p(pc), _p(rgb), n, rgb_bytes, _p(plane), float(distance_threshold), _stream())
    return pc, rgb


def dbscan(points, eps=0.006, min_points=30):
    """points [N,3] f32 -> (labels [N] int32, n_clusters [1] int32) on the device: scikit-learn's DBSCAN labels (docs/preprocessing.md)."""
    _chk(points, torch.float32, "dbscan.points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"dbscan: points must be [N,3], got {tuple(points.shape)}")
    N = points.shape[0]
    labels = torch.empty(N, dtype=torch.int32, device=points.device)
    ncl = torch.zeros(1, dtype=torch.int32, device=points.device)
    if N == 0:      # (an empty tensor has no address to pass)
        return labels, ncl
    ws, wsb = _workspace("cmdiad_dbscan_workspace_bytes", points.device, N)
    _call("cmdiad_dbscan", _p(points), N, float(eps), int(min_points), _p(labels), _p(ncl), _p(ws), wsb, _stream())
    return labels, ncl


def label_histogram(labels, bins):
    """labels [N] int32 -> hist [bins] int32 with hist[b] = count of label b - 1 (bin 0 = noise)."""
    _chk(labels, torch.int32, "label_histogram.labels")
    hist = torch.zeros(int(bins), dtype=torch.int32, device=labels.device)
    if labels.numel() == 0:
        return hist
    _call("cmdiad_label_histogram", _p(labels), labels.numel(), _p(hist), int(bins), _stream())
    return hist


def _scan_window(pc, name):
    """pc [H,W,3] f32 on the device, every row contiguous: a contiguous scan or the window of a larger one -> (H, W, row pitch in floats)."""
    if not pc.is_cuda:
        raise nat.NativeError(f"{name}: tensor must live on the GPU (cmdiad_amd has no CPU path)")
    if pc.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {pc.dtype}")
    if pc.dim() != 3 or pc.shape[2] != 3 or pc.shape[0] < 1 or pc.shape[1] < 1:
        raise ValueError(f"{name}: the scan must be [H,W,3] with H, W >= 1, got {tuple(pc.shape)}")
    H, W, _ = pc.shape
    if pc.stride(2) != 1 or pc.stride(1) != 3 or (H > 1 and pc.stride(0) < 3 * W):
        raise ValueError(f"{name}: every row of the scan must be contiguous, got strides {pc.stride()}")
    return H, W, (pc.stride(0) if H > 1 else 3 * W)


def scan_edges(pc):
    """pc [H,W,3] f32 (contiguous, or the window of a larger scan) -> (points [L,3] f32, count [1] int32) on the device: the valid
    points of get_edges_of_pc's sequence (L entries: first / last 10 rows, first / last 10 columns, corners twice) in its order, in
    points[:count]; the rows past count are not written.  utils/preprocessing.py:20-27."""
    H, W, pitch = _scan_window(pc, "scan_edges.pc")
    L = 2 * min(10, H) * W + 2 * min(10, W) * H
    points = torch.empty((L, 3), dtype=torch.float32, device=pc.device)
    count = torch.empty(1, dtype=torch.int32, device=pc.device)
    ws, wsb = _workspace("cmdiad_scan_edges_workspace_bytes", pc.device, H, W)
    _call("cmdiad_scan_edges", _p(pc), pitch, H, W, _p(points), L, _p(count), _p(ws), wsb, _stream())
    return points, count


def scan_compact(pc):
    """pc [H,W,3] f32 -> (points [H*W,3] f32, index [H*W] int32, count [1] int32) on the device: the valid points in raster order and
    their flat pixel indices in [:count] -- np.nonzero(np.all(pc.reshape(-1, 3) != 0, axis=1)); the rows past count are not written."""
    H, W, pitch = _scan_window(pc, "scan_compact.pc")
    points = torch.empty((H * W, 3), dtype=torch.float32, device=pc.device)
    index = torch.empty(H * W, dtype=torch.int32, device=pc.device)
    count = torch.empty(1, dtype=torch.int32, device=pc.device)
    ws, wsb = _workspace("cmdiad_scan_compact_workspace_bytes", pc.device, H, W)
    _call("cmdiad_scan_compact", _p(pc), pitch, H, W, _p(points), _p(index), H * W, _p(count), _p(ws), wsb, _stream())
    return points, index, count


def keep_largest_cluster(labels, index, hist, n_clusters, pc, rgb=None):
    """In place: pc [...,3] f32 and rgb [..., C] (any dtype, None = xyz only) are zeroed at the pixels index[i] whose labels[i] is not
    the most frequent label of hist [bins] (bin 0 = noise, which can win; ties to the lowest label) -> winner [1] int32 on the device.
    labels, index [N] int32; n_clusters [1] int32 on the device.  utils/preprocessing.py:70-90."""
    _chk(labels, torch.int32, "keep_largest_cluster.labels"); _chk(index, torch.int32, "keep_largest_cluster.index")
    _chk(hist, torch.int32, "keep_largest_cluster.hist"); _chk(n_clusters, torch.int32, "keep_largest_cluster.n_clusters")
    _chk(pc, torch.float32, "keep_largest_cluster.pc")
    N = labels.numel()
    if index.numel() != N:
        raise ValueError(f"keep_largest_cluster: {N} labels, {index.numel()} indices")
    n = pc.numel() // 3
    rgb_bytes = 0
    if rgb is not None:
        if not rgb.is_cuda:
            raise nat.NativeError("keep_largest_cluster.rgb: tensor must live on the GPU (cmdiad_amd has no CPU path)")
        if not rgb.is_contiguous():
            raise ValueError("keep_largest_cluster.rgb: tensor must be contiguous")
        if n == 0 or (rgb.numel() * rgb.element_size()) % n or rgb.numel() // n * n != rgb.numel():
            raise ValueError(f"keep_largest_cluster: rgb {tuple(rgb.shape)} does not match pc {tuple(pc.shape)}")
        rgb_bytes = rgb.numel() * rgb.element_size() // n
    winner = torch.full((1,), -1, dtype=torch.int32, device=pc.device)
    if N == 0 or hist.numel() == 0:      # (an empty tensor has no address to pass)
        return winner
    _call("cmdiad_keep_largest_cluster", _p(labels), _p(index), N, _p(hist), hist.numel(), _p(n_clusters), _p(pc), _p(rgb), n, rgb_bytes,
          _p(winner), _stream())
    return winner


# ------------------------------------------------------------------------------------ sample preparation (docs/sample_prep.md)
def resize_bicubic_u8(src, out_h, out_w, htab, vtab, norm=None, want_u8=False, want_f32=True):
    """src [B,H,W,3] uint8 -> (uint8 [B,out_h,out_w,3] or None, float32 [B,3,out_h,out_w] or None): Pillow's Image.resize(BICUBIC)
    bit for bit, then ToTensor + Normalize through norm [3,256] f32.  htab / vtab = (coef [n_out,ksize] int32, bounds [n_out,2]
    int32) of cmdiad_amd.dataset.bicubic_tables on the device; None for a side that does not change.  dataset.py:62-65."""
    _chk(src, torch.uint8, "resize_bicubic_u8.src"); _chk(norm, torch.float32, "resize_bicubic_u8.norm")
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"resize_bicubic_u8: src must be [B,H,W,3], got {tuple(src.shape)}")
    B, H, W, _ = src.shape
    tabs = []
    for name, tab, n_in, n_out in (("htab", htab, W, out_w), ("vtab", vtab, H, out_h)):
        if n_in == n_out:
            tabs += [None, None, 0]
            continue
        if tab is None:
            raise ValueError(f"resize_bicubic_u8: {name} is needed for {n_in} -> {n_out}")
        coef, bounds = tab
        _chk(coef, torch.int32, f"resize_bicubic_u8.{name}.coef"); _chk(bounds, torch.int32, f"resize_bicubic_u8.{name}.bounds")
        if coef.dim() != 2 or coef.shape[0] != n_out or tuple(bounds.shape) != (n_out, 2):
            raise ValueError(f"resize_bicubic_u8: {name} is {tuple(coef.shape)} / {tuple(bounds.shape)}, {n_out} rows needed")
        tabs += [coef, bounds, coef.shape[1]]
    if want_f32 and norm is None:
        raise ValueError("resize_bicubic_u8: the float output needs the normalise table")
    if norm is not None and tuple(norm.shape) != (3, 256):
        raise ValueError(f"resize_bicubic_u8: norm must be [3,256], got {tuple(norm.shape)}")
    dev = src.device
    tmp = torch.empty((B, H, out_w, 3), dtype=torch.uint8, device=dev) if W != out_w and H != out_h else None
    out_u8 = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    out_f32 = torch.empty((B, 3, out_h, out_w), dtype=torch.float32, device=dev) if want_f32 else None
    _call("cmdiad_resize_bicubic_u8", _p(src), B, H, W, int(out_h), int(out_w), _p(tabs[0]), _p(tabs[1]), tabs[2], _p(tabs[3]),
          _p(tabs[4]), tabs[5], _p(tmp), _p(norm), _p(out_u8), _p(out_f32), _stream())
    return out_u8, out_f32


def _index_pair(tab, H, W, name):
    rows, cols = tab
    _chk(rows, torch.int32, name + ".rows"); _chk(cols, torch.int32, name + ".cols")
    if rows.dim() != 1 or rows.shape != cols.shape:
        raise ValueError(f"{name}: rows / cols must be two [S] tables, got {tuple(rows.shape)} / {tuple(cols.shape)}")
    return rows, cols, rows.shape[0]


def organized_pc_prep(pc, xyz_tab, depth_tab=None):
    """pc [B,H,W,3] f32 or f64 -> (cloud [B,3,xs,xs], depth [B,3,ds,ds] or None, count [B] int32), all float32: the nearest-resized
    cloud, its z channel three times, and the number of resized pixels with three non-zero coordinates.  A float64 cloud (Eyecandies)
    is converted at the gather, round to nearest, as the reference's .float().  xyz_tab / depth_tab = (rows [S], cols [S]) int32
    on the device (cmdiad_amd.dataset.torch_nearest_index).  dataset.py:106-111."""
    if pc.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"organized_pc_prep.pc: expected torch.float32 or torch.float64, got {pc.dtype}")
    _chk(pc, pc.dtype, "organized_pc_prep.pc")
    if pc.dim() != 4 or pc.shape[3] != 3:
        raise ValueError(f"organized_pc_prep: pc must be [B,H,W,3], got {tuple(pc.shape)}")
    B, H, W, _ = pc.shape
    rows, cols, xs = _index_pair(xyz_tab, H, W, "organized_pc_prep.xyz_tab")
    drows = dcols = depth = None
    ds = 0
    if depth_tab is not None:
        drows, dcols, ds = _index_pair(depth_tab, H, W, "organized_pc_prep.depth_tab")
        depth = torch.empty((B, 3, ds, ds), dtype=torch.float32, device=pc.device)
    cloud = torch.empty((B, 3, xs, xs), dtype=torch.float32, device=pc.device)
    count = torch.empty((B,), dtype=torch.int32, device=pc.device)
    _call("cmdiad_organized_pc_prep_f64" if pc.dtype == torch.float64 else "cmdiad_organized_pc_prep", _p(pc), B, H, W, _p(rows), _p(cols), xs, _p(drows), _p(dcols), ds, _p(cloud), _p(depth),
          _p(count), _stream())
    return cloud, depth, count


def gt_mask_prep(gt, tab):
    """gt [B,H,W] uint8 -> [B,1,gs,gs] f32 in {0, 1}: Pillow's NEAREST resize through tab = (rows [gs], cols [gs]) int32 on the device
    (cmdiad_amd.dataset.pillow_nearest_index), / 255, > 0.5.  dataset.py:168-171, 239-241."""
    _chk(gt, torch.uint8, "gt_mask_prep.gt")
    if gt.dim() != 3:
        raise ValueError(f"gt_mask_prep: gt must be [B,H,W], got {tuple(gt.shape)}")
    B, H, W = gt.shape
    rows, cols, gs = _index_pair(tab, H, W, "gt_mask_prep.tab")
    out = torch.empty((B, 1, gs, gs), dtype=torch.float32, device=gt.device)
    _call("cmdiad_gt_mask_prep", _p(gt), B, H, W, _p(rows), _p(cols), gs, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------ xyz TIFFs (docs/tiff.md)
TIFF_MAX_ROW_BYTES = 64 * 1024     # the longest predictor-3 chunk row cmdiad_tiff_unpack undoes (utils.tiff undoes longer ones on the host)


def tiff_unpack(raw_u8, layouts, chunk_table, table_dev=None, out=None):
    """raw_u8 [n] uint8 on the device (file bytes with uncompressed chunks; n a multiple of 4), layouts = the utils.tiff.TiffLayout of
    every image (equal but for their offsets), chunk_table [B, n_chunks] int64 ON THE HOST = every chunk's byte offset into raw_u8
    -> [B,H,W,C] float32 or float64, the files' samples bit for bit.  The table is checked here, before the launch, against the
    geometry and raw_u8's length: a chunk that starts before 0 or ends past the buffer is a ValueError and nothing is launched.
    table_dev: the same table already on the device (else it is uploaded here); out: the result tensor to fill."""
    import numpy as np
    _chk(raw_u8, torch.uint8, "tiff_unpack.raw_u8")
    layouts = list(layouts)
    if not layouts:
        raise ValueError("tiff_unpack: no layouts")
    lay = layouts[0]
    B, n = len(layouts), lay.n_chunks
    if any(l.geometry() != lay.geometry() for l in layouts):
        raise ValueError("tiff_unpack: the layouts of one call must be equal but for their offsets")
    if lay.compression != 1:
        raise ValueError(f"tiff_unpack: chunks must be uncompressed (utils.tiff.read_raw inflates them), got compression {lay.compression}")
    if lay.predictor == 3 and lay.row_bytes > TIFF_MAX_ROW_BYTES:
        raise ValueError(f"tiff_unpack: a predictor-3 chunk row of {lay.row_bytes} bytes exceeds {TIFF_MAX_ROW_BYTES}: undo it on the host")
    table = np.ascontiguousarray(chunk_table.numpy() if isinstance(chunk_table, torch.Tensor) else chunk_table, dtype=np.int64)
    if table.shape != (B, n):
        raise ValueError(f"tiff_unpack: chunk_table must be [{B},{n}] for this geometry, got {table.shape}")
    raw_bytes = raw_u8.numel()
    if raw_u8.dim() != 1 or raw_bytes == 0 or raw_bytes % 4 or raw_u8.data_ptr() % 4:
        raise ValueError(f"tiff_unpack: raw_u8 must be a dword-aligned 1-D buffer padded to a multiple of 4 bytes, got {tuple(raw_u8.shape)}")
    need = lay.all_chunk_bytes()
    bad = np.argwhere((table < 0) | (table + need[None, :] > raw_bytes))
    if len(bad):
        b, k = (int(v) for v in bad[0])
        raise ValueError(f"tiff_unpack: chunk {k} of image {b} at offset {int(table[b, k])} with {int(need[k])} bytes does not lie inside "
                         f"the {raw_bytes} bytes of raw_u8")
    dtype = torch.float32 if lay.bytes_per_sample == 4 else torch.float64
    shape = (B, lay.height, lay.width, lay.channels)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=raw_u8.device)
    else:
        _chk(out, dtype, "tiff_unpack.out")
        if tuple(out.shape) != shape:
            raise ValueError(f"tiff_unpack: out must be {shape}, got {tuple(out.shape)}")
    if table_dev is None:
        table_dev = torch.from_numpy(table).to(raw_u8.device)
    _chk(table_dev, torch.int64, "tiff_unpack.table_dev")
    if tuple(table_dev.shape) != (B, n):
        raise ValueError(f"tiff_unpack: table_dev must be [{B},{n}], got {tuple(table_dev.shape)}")
    _call("cmdiad_tiff_unpack", _p(raw_u8), raw_bytes, _p(table_dev), B, n, lay.width, lay.height, lay.channels, lay.chunk_w, lay.chunk_h,
          int(lay.planar), lay.bytes_per_sample, int(lay.big_endian), lay.predictor, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------ PNGs (docs/png.md)
PNG_TARGETS = ("rgb", "l", "raw")     # the index is cmdiad_png_unfilter's target code


def png_unfilter(raw_u8, layouts, offsets, target, out=None, offsets_dev=None, waves=0):
    """raw_u8 [n] uint8 on the device (inflated, still filtered scanlines), layouts = the utils.png.PngLayout of every image (equal
    width, height and bytes per pixel; 8-bit, colour type 0 / 2 / 4 / 6), offsets [B] int64 ON THE HOST = where every image's
    scanlines start in raw_u8, target 'rgb' | 'l' | 'raw' -> uint8 [B,H,W,3] | [B,H,W] | [B,H,W,C] ([B,H,W] for one channel), bit
    for bit what Pillow decodes and converts.  Every image's [offset, offset + H * (1 + row_bytes)) is checked here against the
    buffer: a bad one is a ValueError and nothing is launched.  offsets_dev: the same table already on the device (else it is
    uploaded here); out: the result tensor to fill; waves: 0 = chosen from the width, 1 = the one-wave baseline (tools/bench_png.py)."""
    import numpy as np
    _chk(raw_u8, torch.uint8, "png_unfilter.raw_u8")
    layouts = list(layouts)
    if not layouts:
        raise ValueError("png_unfilter: no layouts")
    if target not in PNG_TARGETS:
        raise ValueError(f"png_unfilter: target must be one of {PNG_TARGETS}, got {target!r}")
    lay = layouts[0]
    B = len(layouts)
    if any(l.geometry() != lay.geometry() for l in layouts):
        raise ValueError("png_unfilter: the layouts of one call must share width, height and bytes per pixel")
    if lay.bit_depth != 8 or lay.color_type not in (0, 2, 4, 6) or lay.interlace or lay.row_bytes != lay.width * lay.bpp:
        raise ValueError(f"png_unfilter: 8-bit non-interlaced files of colour type 0 / 2 / 4 / 6 only, got bit depth {lay.bit_depth}, "
                         f"colour type {lay.color_type}, interlace {lay.interlace}")
    table = np.ascontiguousarray(offsets.numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
    if table.shape != (B,):
        raise ValueError(f"png_unfilter: offsets must be [{B}], got {table.shape}")
    raw_bytes = raw_u8.numel()
    if raw_u8.dim() != 1 or raw_bytes == 0:
        raise ValueError(f"png_unfilter: raw_u8 must be a non-empty 1-D buffer, got {tuple(raw_u8.shape)}")
    need = lay.height * (1 + lay.row_bytes)
    bad = np.flatnonzero((table < 0) | (table + need > raw_bytes))
    if len(bad):
        b = int(bad[0])
        raise ValueError(f"png_unfilter: image {b} at offset {int(table[b])} with {need} bytes of scanlines does not lie inside the "
                         f"{raw_bytes} bytes of raw_u8")
    H, W, C = lay.height, lay.width, lay.channels
    shape = (B, H, W, 3) if target == "rgb" else (B, H, W) if target == "l" or C == 1 else (B, H, W, C)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=raw_u8.device)
    else:
        _chk(out, torch.uint8, "png_unfilter.out")
        if tuple(out.shape) != shape:
            raise ValueError(f"png_unfilter: out must be {shape}, got {tuple(out.shape)}")
    if offsets_dev is None:
        offsets_dev = torch.from_numpy(table).to(raw_u8.device)
    _chk(offsets_dev, torch.int64, "png_unfilter.offsets_dev")
    if tuple(offsets_dev.shape) != (B,):
        raise ValueError(f"png_unfilter: offsets_dev must be [{B}], got {tuple(offsets_dev.shape)}")
    _call("cmdiad_png_unfilter", _p(raw_u8), raw_bytes, _p(offsets_dev), B, W, H, lay.bpp, PNG_TARGETS.index(target), int(waves), _p(out),
          _stream())
    return out


# ------------------------------------------------------------------------------------ Eyecandies (docs/eyecandies.md)
EYECANDIES_PARAM_BYTES = 136     # cmdiad_eyecandies_params: float32 range, float32 mind, float64 inv(P)[16]


def eyecandies_params(mind, maxd, inv_p):
    """One scan's parameter block on the HOST: uint8 [136] = float32(maxd - mind) (subtracted in double first), float32(mind), and
    inv_p [4,4] float64 (numpy.linalg.inv(K4 @ pose)), as cmdiad_eyecandies_params lays them out."""
    import numpy as np
    inv_p = np.asarray(inv_p, dtype=np.float64)
    if inv_p.shape != (4, 4):
        raise ValueError(f"eyecandies_params: inv_p must be [4,4], got {inv_p.shape}")
    blk = np.empty(EYECANDIES_PARAM_BYTES, dtype=np.uint8)
    blk[0:8].view(np.float32)[:] = (np.float32(float(maxd) - float(mind)), np.float32(float(mind)))
    blk[8:].view(np.float64)[:] = inv_p.reshape(16)
    return torch.from_numpy(blk)


def _chk_eyecandies(depth_u16, params, name):
    _chk(depth_u16, torch.uint16, name + ".depth_u16"); _chk(params, torch.uint8, name + ".params")
    if depth_u16.dim() != 3:
        raise ValueError(f"{name}: depth_u16 must be [B,H,W], got {tuple(depth_u16.shape)}")
    B, H, W = depth_u16.shape
    if tuple(params.shape) != (B, EYECANDIES_PARAM_BYTES):
        raise ValueError(f"{name}: params must be [{B},{EYECANDIES_PARAM_BYTES}] uint8 (eyecandies_params per scan), got {tuple(params.shape)}")
    return B, H, W


def eyecandies_cloud(depth_u16, params, want_removed=True, want_depth=False):
    """depth_u16 [B,H,W] uint16 (the PNG codes), params [B,136] uint8 (eyecandies_params) -> (cloud [B,H,W,3] f64, removed [B,H,W] u8
    or None, depth [B,H,W] f32 or None): the reference's depth_to_pointcloud + remove_point_cloud_background in one launch; a removed
    point is the reference's collapsed point, not zero.  utils/preprocessing_eyecandies.py:16-89."""
    B, H, W = _chk_eyecandies(depth_u16, params, "eyecandies_cloud")
    dev = depth_u16.device
    cloud = torch.empty((B, H, W, 3), dtype=torch.float64, device=dev)
    removed = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_removed else None
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    _call("cmdiad_eyecandies_cloud", _p(depth_u16), _p(params), B, H, W, _p(cloud), _p(removed), _p(depth), _stream())
    return cloud, removed, depth


def eyecandies_unproject(depth_u16, params, want_points=True, want_depth=False):
    """The first stage alone -> (points [B,H*W,3] f64 or None, depth [B,H,W] f32 or None): depth_to_pointcloud / load_and_convert_depth
    (utils/preprocessing_eyecandies.py:16-59)."""
    B, H, W = _chk_eyecandies(depth_u16, params, "eyecandies_unproject")
    dev = depth_u16.device
    points = torch.empty((B, H * W, 3), dtype=torch.float64, device=dev) if want_points else None
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    _call("cmdiad_eyecandies_unproject", _p(depth_u16), _p(params), B, H, W, _p(points), _p(depth), _stream())
    return points, depth


def eyecandies_background(points):
    """points [n,3] f64 -> (cloud [n,3] f64, removed [n] u8): remove_point_cloud_background (utils/preprocessing_eyecandies.py:62-89)."""
    _chk(points, torch.float64, "eyecandies_background.points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"eyecandies_background: points must be [n,3], got {tuple(points.shape)}")
    n = points.shape[0]
    cloud = torch.empty_like(points)
    removed = torch.empty((n,), dtype=torch.uint8, device=points.device)
    _call("cmdiad_eyecandies_background", _p(points), n, _p(cloud), _p(removed), _stream())
    return cloud, removed


# ------------------------------------------------------------------------------------ pixel metrics (docs/metrics.md)
SORT_TILE = 4096          # keys per block of a radix pass (cmdiad_sort_u64_tile): sizes around its multiples change the passes' shape
PRO_MAX_THRESHOLDS = 1024  # cmdiad_pro_hist keeps the thresholds in LDS
# (the u64 keys travel in int64 tensors, bit for bit, as the search keys do: torch indexes and copies int64 everywhere)


def ccl_label(masks):
    """masks [n,H,W] float32 or uint8 (foreground = non-zero) -> (labels [n,H,W] i32, n_comp [n] i32, comp_offset [n+1] i32,
    comp_size [n ceil(H/2) ceil(W/2)] i32 -- zero past comp_offset[n] entries --, nonbinary [1] i32 = values neither 0 nor 1).
    8-connected, numbered as scipy.ndimage.label(mask, ones((3,3))) numbers them.  No synchronisation."""
    if masks.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"ccl_label.masks: expected torch.float32 or torch.uint8, got {masks.dtype}")
    n, H, W = _chk_maps(masks, "ccl_label", "masks", masks.dtype)
    dev = masks.device
    cap = n * ((H + 1) // 2) * ((W + 1) // 2)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    n_comp = torch.empty((n,), dtype=torch.int32, device=dev)
    comp_offset = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
    comp_size = torch.empty((cap,), dtype=torch.int32, device=dev)
    nonbinary = torch.zeros((1,), dtype=torch.int32, device=dev)
    if n == 0:
        return labels, n_comp, comp_offset, comp_size, nonbinary
    ws, wsb = _workspace("cmdiad_ccl_workspace_bytes", dev, n, H, W)
    _call("cmdiad_ccl_label", _p(masks), int(masks.dtype == torch.uint8), n, H, W, _p(labels), _p(n_comp), _p(comp_offset),
          _p(comp_size), cap, _p(nonbinary), _p(ws), wsb, _stream())
    return labels, n_comp, comp_offset, comp_size, nonbinary


def _chk_list(t, dtype, name):
    _chk(t, dtype, name)
    if t.dim() != 1 or t.numel() > FRAME_MAX_TOTAL:
        raise ValueError(f"{name}: must be one-dimensional with at most 2^30 entries, got {tuple(t.shape)}")
    return t.numel()


def f64_to_keys(x):
    """x [n] f64 -> (keys [n] u64 in the order of the doubles, -0.0 taken as +0.0; nonfinite [1] i32 = NaN / infinite inputs)."""
    n = _chk_list(x, torch.float64, "f64_to_keys.x")
    keys = torch.empty((n,), dtype=torch.int64, device=x.device)
    nonfinite = torch.zeros((1,), dtype=torch.int32, device=x.device)
    if n:
        _call("cmdiad_f64_to_keys", _p(x), n, _p(keys), _p(nonfinite), _stream())
    return keys, nonfinite


def keys_to_f64(keys):
    """The inverse of f64_to_keys: keys [n] u64 -> [n] f64."""
    n = _chk_list(keys, torch.int64, "keys_to_f64.keys")
    out = torch.empty((n,), dtype=torch.float64, device=keys.device)
    if n:
        _call("cmdiad_keys_to_f64", _p(keys), n, _p(out), _stream())
    return out


def sort_u64_(keys):
    """keys [n] u64, sorted ascending IN PLACE (LSD radix sort, keys only); returns keys."""
    n = _chk_list(keys, torch.int64, "sort_u64_.keys")
    if n:
        ws, wsb = _workspace("cmdiad_sort_u64_workspace_bytes", keys.device, n)
        _call("cmdiad_sort_u64", _p(keys), n, _p(ws), wsb, _stream())
    return keys


def metrics_split(preds, labels, comp_offset, ok_cap, def_cap):
    """preds [n,H,W] f64 + the labels / comp_offset of ccl_label -> (ok_keys [ok_cap] u64, def_score [def_cap] f64, def_comp [def_cap]
    i32, counts [2] i64 = true lengths of the two lists, nonfinite [1] i32).  The order inside the lists is not defined."""
    _chk(preds, torch.float64, "metrics_split.preds"); _chk(labels, torch.int32, "metrics_split.labels")
    _chk(comp_offset, torch.int32, "metrics_split.comp_offset")
    if preds.dim() != 3 or preds.shape != labels.shape or comp_offset.numel() != preds.shape[0] + 1:
        raise ValueError(f"metrics_split: preds {tuple(preds.shape)} and labels {tuple(labels.shape)} must be the same [n,H,W], "
                         f"comp_offset [n+1] (got {comp_offset.numel()})")
    refusal = f"metrics_split: unsupported sizes {tuple(preds.shape)} ok_cap={ok_cap} def_cap={def_cap}"
    n, H, W = _frames(preds.shape, "metrics_split", least=0, msg=refusal)
    total = n * H * W
    if not (0 <= ok_cap <= total and 0 <= def_cap <= total):
        raise ValueError(refusal)
    dev = preds.device
    ok_keys = torch.empty((ok_cap,), dtype=torch.int64, device=dev)
    def_score = torch.empty((def_cap,), dtype=torch.float64, device=dev)
    def_comp = torch.empty((def_cap,), dtype=torch.int32, device=dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    nonfinite = torch.zeros((1,), dtype=torch.int32, device=dev)
    if total:
        _call("cmdiad_metrics_split", _p(preds), _p(labels), _p(comp_offset), n, H * W, _p(ok_keys), ok_cap, _p(def_score),
              _p(def_comp), def_cap, _p(counts), _p(nonfinite), _stream())
    return ok_keys, def_score, def_comp, counts, nonfinite


def auc_counts(ok_sorted_keys, def_score):
    """-> S [1] i64 = sum over the defect scores s of #(ok < s) + #(ok <= s); ok_sorted_keys: the SORTED keys of the defect-free scores."""
    n_ok = _chk_list(ok_sorted_keys, torch.int64, "auc_counts.ok_sorted_keys")
    n_def = _chk_list(def_score, torch.float64, "auc_counts.def_score")
    S = torch.zeros((1,), dtype=torch.int64, device=def_score.device)
    if n_ok and n_def:
        _call("cmdiad_auc_counts", _p(ok_sorted_keys), n_ok, _p(def_score), n_def, _p(S), _stream())
    return S


def pro_hist(thr, def_score, def_comp, total_comp):
    """thr [T] f64 ascending (T <= 1024) -> hist [total_comp, T+1] i32: hist[c][b] = defect pixels of component c with exactly b
    thresholds strictly below their score."""
    T = _chk_list(thr, torch.float64, "pro_hist.thr")
    n_def = _chk_list(def_score, torch.float64, "pro_hist.def_score")
    if _chk_list(def_comp, torch.int32, "pro_hist.def_comp") != n_def:
        raise ValueError("pro_hist: def_score and def_comp differ in length")
    if T > PRO_MAX_THRESHOLDS:
        raise ValueError(f"pro_hist: {T} thresholds, at most {PRO_MAX_THRESHOLDS}")
    if total_comp < 0 or total_comp * (T + 1) > (1 << 28):
        raise ValueError(f"pro_hist: a table of {total_comp} components x {T + 1} bins is above 2^28 entries (1 GiB)")
    hist = torch.zeros((total_comp, T + 1), dtype=torch.int32, device=def_score.device)
    if n_def and total_comp:
        _call("cmdiad_pro_hist", _p(thr), T, _p(def_score), _p(def_comp), n_def, total_comp, _p(hist), _stream())
    return hist


# ------------------------------------------------------------------------------------ defect regions (docs/regions.md)
REGION_MAX = 64          # cmdiad_region_table: slots per image


def threshold_mask(maps, thr, mask=None, nan_count=None):
    """maps [n,H,W] f64, thr f64 ON THE DEVICE with 1 or n entries -> (mask [n,H,W] u8 = maps > thr, nan_count [1] i32 = NaN scores,
    which stay background).  -0.0 > +0.0 is false.  The threshold is read by the kernel: rewriting `thr` in place changes what the
    next launch (or graph replay) computes.  mask / nan_count: buffers to write into.  No synchronisation."""
    n, H, W = _chk_maps(maps, "threshold_mask")
    _chk(thr, torch.float64, "threshold_mask.thr")
    if thr.numel() not in (1, n) or thr.device != maps.device:
        raise ValueError(f"threshold_mask: thr must hold 1 or n = {n} values on the maps' device, got {tuple(thr.shape)} on {thr.device}")
    mask = _out(mask, torch.uint8, (n, H, W), maps.device, "threshold_mask.mask")
    nan_count = _out(nan_count, torch.int32, (1,), maps.device, "threshold_mask.nan_count", zero=True)
    if n:
        _call("cmdiad_threshold_mask", _p(maps), _p(thr), int(thr.numel() == n and n > 1), n, H, W, _p(mask), _p(nan_count), _stream())
    return mask, nan_count


def region_table(maps, labels, n_comp, comp_offset, comp_size, min_area=1, max_regions=16):
    """maps [n,H,W] f64 + the outputs of ccl_label on their mask -> (count [n] i32 = components with area >= min_area, ints
    [n,K,8] i32 = label, area, x0, y0, x1, y1, peak_x, peak_y, vals [n,K,4] f64 = peak, score_sum, cx, cy) of the first K =
    max_regions of them by (peak descending, label ascending); zero behind the last region, count > K = truncated.  No
    synchronisation, nothing is read back."""
    min_area, K = int(min_area), int(max_regions)
    if min_area < 1 or not 1 <= K <= REGION_MAX:
        raise ValueError(f"region_table: min_area = {min_area} (>= 1), max_regions = {K} (1..{REGION_MAX})")
    n, H, W = _chk_maps(maps, "region_table")
    _chk(labels, torch.int32, "region_table.labels"); _chk(n_comp, torch.int32, "region_table.n_comp")
    _chk(comp_offset, torch.int32, "region_table.comp_offset"); _chk(comp_size, torch.int32, "region_table.comp_size")
    cap = n * ((H + 1) // 2) * ((W + 1) // 2)
    if labels.shape != maps.shape or n_comp.numel() != n or comp_offset.numel() != n + 1 or comp_size.numel() < cap:
        raise ValueError(f"region_table: maps {tuple(maps.shape)} need labels of that shape, n_comp [n], comp_offset [n+1] and comp_size "
                         f"[>= {cap}]; got {tuple(labels.shape)}, {n_comp.numel()}, {comp_offset.numel()}, {comp_size.numel()}")
    dev = maps.device
    _on_device(dev, "region_table", labels=labels, n_comp=n_comp, comp_offset=comp_offset, comp_size=comp_size)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    ints = torch.zeros((n, K, 8), dtype=torch.int32, device=dev)
    vals = torch.zeros((n, K, 4), dtype=torch.float64, device=dev)
    if n:
        ws, wsb = _workspace("cmdiad_region_table_workspace_bytes", dev, n, H, W)
        _call("cmdiad_region_table", _p(maps), _p(labels), _p(n_comp), _p(comp_offset), _p(comp_size), comp_size.numel(), n, H, W,
              min_area, K, _p(count), _p(ints), _p(vals), _p(ws), wsb, _stream())
    return count, ints, vals


# ------------------------------------------------------------------------------------ precision-recall, detection counts (docs/metrics.md)
PR_TILE = 2048            # keys per block of the run-head passes (cmdiad_pr_tile): sizes around its multiples change the passes' shape
PR_F1_BLOCK = 256         # runs per block-step of cmdiad_pr_f1max's first stage: runs 256 j .. 256 j + 255 meet in one block
PR_F1_MAX_BLOCKS = 1024   # ... and block b takes j = b, b + blocks, ... with blocks = min(ceil(run_cap / 256), 1024)


def pr_runs(def_sorted_keys, ok_sorted_keys):
    """The SORTED keys of the defect scores [n_def] and of the defect-free scores [n_ok] -> (run_key [n_def] u64, run_first [n_def]
    i32, run_fp [n_def] i32, n_runs [1] i32): per run of equal defect keys, in ascending key order, the key, the index of its first
    element and the number of defect-free scores at or above it.  Entries past n_runs are not written.  No synchronisation."""
    n_def = _chk_list(def_sorted_keys, torch.int64, "pr_runs.def_sorted_keys")
    n_ok = _chk_list(ok_sorted_keys, torch.int64, "pr_runs.ok_sorted_keys")
    dev = def_sorted_keys.device
    _on_device(dev, "pr_runs", ok_sorted_keys=ok_sorted_keys)
    run_key = torch.empty((n_def,), dtype=torch.int64, device=dev)
    run_first = torch.empty((n_def,), dtype=torch.int32, device=dev)
    run_fp = torch.empty((n_def,), dtype=torch.int32, device=dev)
    n_runs = torch.zeros((1,), dtype=torch.int32, device=dev)
    if n_def:
        tile_heads = torch.empty((2 * -(-n_def // PR_TILE),), dtype=torch.int32, device=dev)      # heads per tile | their scan
        _call("cmdiad_pr_runs", _p(def_sorted_keys), n_def, _p(ok_sorted_keys), n_ok, _p(run_key), _p(run_first), _p(run_fp), n_def,
              _p(n_runs), _p(tile_heads), tile_heads.numel(), _stream())
    return run_key, run_first, run_fp, n_runs


def pr_f1max(run_first, run_fp, n_runs, n_def):
    """A run table as plain integers (run_first, run_fp [cap] i32, n_runs [1] i32 on the device, n_def) -> best [2] i64 = (the run
    that maximises 2 tp / (tp + fp + n_def), tp = n_def - run_first, compared exactly, the largest index among equals; 0).  -1 when
    the table holds no run.  No synchronisation."""
    cap = _chk_list(run_first, torch.int32, "pr_f1max.run_first")
    if _chk_list(run_fp, torch.int32, "pr_f1max.run_fp") != cap:
        raise ValueError("pr_f1max: run_first and run_fp differ in length")
    _chk(n_runs, torch.int32, "pr_f1max.n_runs")
    n_def = int(n_def)
    if n_runs.numel() != 1 or not 0 <= n_def <= FRAME_MAX_TOTAL:
        raise ValueError(f"pr_f1max: n_runs must hold one entry and n_def = {n_def} lie in 0..2^30")
    dev = run_first.device
    _on_device(dev, "pr_f1max", run_fp=run_fp, n_runs=n_runs)
    best = torch.tensor([-1, 0], dtype=torch.int64, device=dev)
    if cap:
        partial = torch.empty((min(-(-cap // PR_F1_BLOCK), PR_F1_MAX_BLOCKS),), dtype=torch.int32, device=dev)   # the first stage's winners
        _call("cmdiad_pr_f1max", _p(run_first), _p(run_fp), _p(n_runs), cap, n_def, _p(best), _p(partial), partial.numel(), _stream())
    return best


def _chk_labelling(labels, comp_offset, who, what):
    _chk(labels, torch.int32, f"{who}.{what}_labels"); _chk(comp_offset, torch.int32, f"{who}.{what}_comp_offset")
    if labels.dim() != 3 or comp_offset.numel() != labels.shape[0] + 1:
        raise ValueError(f"{who}: {what}_labels must be [n,H,W] and {what}_comp_offset [n+1], got {tuple(labels.shape)} and "
                         f"{comp_offset.numel()}")


def region_overlap(gt_labels, gt_comp_offset, pred_labels, pred_comp_offset, pred_comp_size, min_area=1):
    """Two labellings of the same frames (ccl_label's outputs) -> (covered [n ceil(H/2) ceil(W/2)] i32 per ground-truth component = its
    pixels inside a predicted component of at least min_area pixels, hits [len(pred_comp_size)] i32 per predicted component = the
    ground-truth pixels inside it, 0 when it is smaller than min_area).  No synchronisation."""
    min_area = int(min_area)
    if min_area < 1:
        raise ValueError(f"region_overlap: min_area = {min_area} (>= 1)")
    _chk_labelling(gt_labels, gt_comp_offset, "region_overlap", "gt")
    _chk_labelling(pred_labels, pred_comp_offset, "region_overlap", "pred")
    _chk(pred_comp_size, torch.int32, "region_overlap.pred_comp_size")
    n, H, W = _frames(gt_labels.shape, "region_overlap")
    if pred_labels.shape != gt_labels.shape or pred_comp_size.dim() != 1:
        raise ValueError(f"region_overlap: gt_labels {tuple(gt_labels.shape)} and pred_labels {tuple(pred_labels.shape)} must be the same "
                         "[n,H,W], pred_comp_size one-dimensional")
    dev = gt_labels.device
    _on_device(dev, "region_overlap", gt_comp_offset=gt_comp_offset, pred_labels=pred_labels, pred_comp_offset=pred_comp_offset,
               pred_comp_size=pred_comp_size)
    covered = torch.zeros((n * ((H + 1) // 2) * ((W + 1) // 2),), dtype=torch.int32, device=dev)
    hits = torch.zeros((pred_comp_size.numel(),), dtype=torch.int32, device=dev)
    if n:
        _call("cmdiad_region_overlap", _p(gt_labels), _p(gt_comp_offset), covered.numel(), _p(pred_labels), _p(pred_comp_offset),
              _p(pred_comp_size), hits.numel(), n, H, W, min_area, _p(covered), _p(hits), _stream())
    return covered, hits


def detection_counts(gt_comp_offset, covered, pred_comp_offset, pred_comp_size, hits, min_area=1):
    """region_overlap's tables -> counts [n,4] i32 per image: ground-truth components, those with covered > 0, predicted components
    of at least min_area pixels, those of them with hits == 0.  No synchronisation."""
    min_area = int(min_area)
    if min_area < 1:
        raise ValueError(f"detection_counts: min_area = {min_area} (>= 1)")
    for t, name in ((gt_comp_offset, "gt_comp_offset"), (covered, "covered"), (pred_comp_offset, "pred_comp_offset"),
                    (pred_comp_size, "pred_comp_size"), (hits, "hits")):
        _chk_list(t, torch.int32, f"detection_counts.{name}")
    n = gt_comp_offset.numel() - 1
    if n < 0 or n > FRAME_MAX_IMAGES or pred_comp_offset.numel() != n + 1 or hits.numel() != pred_comp_size.numel():
        raise ValueError(f"detection_counts: gt_comp_offset and pred_comp_offset must both be [n+1] (n <= {FRAME_MAX_IMAGES}), hits as long as "
                         f"pred_comp_size; got {gt_comp_offset.numel()}, {pred_comp_offset.numel()}, {hits.numel()}, {pred_comp_size.numel()}")
    dev = gt_comp_offset.device
    _on_device(dev, "detection_counts", covered=covered, pred_comp_offset=pred_comp_offset, pred_comp_size=pred_comp_size, hits=hits)
    counts = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    if n:
        _call("cmdiad_detection_counts", _p(gt_comp_offset), _p(covered), covered.numel(), _p(pred_comp_offset), _p(pred_comp_size),
              _p(hits), hits.numel(), n, min_area, _p(counts), _stream())
    return counts


def cloud_layout(cloud, H, W, layout=None, who="region_measure"):
    """'planar' ([n,3,H,W]) or 'interleaved' ([n,H,W,3]) for an organised cloud beside maps of H x W.  The shape decides; a
    [n,3,H,W] cloud with H == 3 or W == 3 can be read both ways and is refused unless `layout` names one."""
    if layout not in (None, "planar", "interleaved"):
        raise ValueError(f"{who}: layout must be 'planar', 'interleaved' or None, got {layout!r}")
    if cloud.dim() != 4:
        raise ValueError(f"{who}: the cloud must be [n,3,{H},{W}] or [n,{H},{W},3], got {tuple(cloud.shape)}")
    fits = [name for name, shape in (("planar", (3, H, W)), ("interleaved", (H, W, 3))) if tuple(cloud.shape[1:]) == shape]
    if layout is not None:
        if layout not in fits:
            raise ValueError(f"{who}: a {layout} cloud beside {H} x {W} maps cannot have the shape {tuple(cloud.shape)}")
        return layout
    if not fits:
        raise ValueError(f"{who}: the cloud must be [n,3,{H},{W}] or [n,{H},{W},3] like the maps, got {tuple(cloud.shape)}")
    if len(fits) == 2 or (fits[0] == "planar" and 3 in (H, W)):
        raise ValueError(f"{who}: a cloud of shape {tuple(cloud.shape)} can be read as planar and as interleaved; pass layout=")
    return fits[0]


def region_measure(labels, count, ints, cloud, out=None, layout=None):
    """labels [n,H,W] i32, count [n] i32, ints [n,K,8] i32 (ccl_label / region_table) and the organised cloud of the maps, f32,
    planar [n,3,H,W] or interleaved [n,H,W,3] (worked out from the shape; layout= where H or W is 3) -> (m_ints [n,K,4] i32 = n_pts,
    n_tri, peak_valid, 0; m_vals [n,K,20] f64 = lo, hi, peak_xyz, s1, s2, area, 0; bad_count [1] i32 = points with a non-finite
    coordinate).  out: that triple, to write into.  docs/regions.md has the contract.  No synchronisation."""
    n, H, W = _chk_maps(labels, "region_measure", "labels", torch.int32)
    K = _chk_region_tables(count, ints, n, "region_measure")
    _chk(cloud, torch.float32, "region_measure.cloud")
    planar = cloud_layout(cloud, H, W, layout) == "planar"
    if cloud.shape[0] != n:
        raise ValueError(f"region_measure: {cloud.shape[0]} clouds for {n} label images")
    dev = labels.device
    _on_device(dev, "region_measure", count=count, ints=ints, cloud=cloud)
    m_ints, m_vals, bad_count = out or (None, None, None)
    m_ints = _out(m_ints, torch.int32, (n, K, 4), dev, "region_measure.m_ints")
    m_vals = _out(m_vals, torch.float64, (n, K, 20), dev, "region_measure.m_vals")
    bad_count = _out(bad_count, torch.int32, (1,), dev, "region_measure.bad_count", zero=True)
    _call("cmdiad_region_measure", _p(labels), _p(count), _p(ints), _p(cloud), 1 if planar else 3, H * W if planar else 1, n, H, W, K,
          _p(m_ints), _p(m_vals), _p(bad_count), _stream())
    return m_ints, m_vals, bad_count


# ------------------------------------------------------------------------------------ overlays (docs/overlay.md)
OVERLAY_BACKGROUNDS = (None, torch.uint8, torch.float32)     # the index is cmdiad_overlay_render's background kind
PNG_FILTER_MODES = ("none", "sub", "up", "average", "paeth", "adaptive")     # the index is cmdiad_png_filter's mode


def _rgb_word(rgb, who):
    r, g, b = (int(v) for v in rgb)
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"{who}: a colour is three bytes, got {tuple(rgb)!r}")
    return r | g << 8 | b << 16


def overlay_render(maps, lohi, lut, alpha, size=None, thr=None, background=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                   count=None, ints=None, line_px=1, contour_rgb=(255, 255, 255), box_rgb=(0, 255, 0), canvas=None, nan_count=None):
    """maps [n,H,W] f64 -> (canvas [n,Ho,Wo,3] u8, nan_count [1] i32), one launch (include/cmdiad_hip.h has the arithmetic).
    lohi: f64 ON THE DEVICE, [2] or [n,2]; thr: None (no contour) or f64 on the device with 1 or n entries -- both are read by
    the kernel, rewriting them in place changes the next launch.  lut [256,3] u8 and alpha [256] u8 on the device.  size = (Ho, Wo),
    default the map's.  background: None, uint8 [n,Ho,Wo,3], or float32 [n,3,Ho,Wo] normalised with mean / std.  count [n] i32 and
    ints [n,K,8] i32: cmdiad_region_table's tables (both or neither).  canvas / nan_count: buffers to write into.  No
    synchronisation."""
    n, H, W = _chk_maps(maps, "overlay_render")
    dev = maps.device
    Ho, Wo = (H, W) if size is None else (int(size[0]), int(size[1]))
    refusal = f"overlay_render: maps {tuple(maps.shape)} -> canvas {Ho} x {Wo}: sides 1..2^14, n*Ho*Wo <= 2^30"
    _frames(maps.shape, "overlay_render", side=FRAME_MAX_SIDE, msg=refusal)
    _frames((n, Ho, Wo), "overlay_render", side=FRAME_MAX_SIDE, pixels=None, msg=refusal)
    kind, lohi_per_image, mean, std = _chk_colours("overlay_render", n, Ho, Wo, lohi, lut, alpha, background, mean, std)
    _chk(thr, torch.float64, "overlay_render.thr")
    if thr is not None and thr.numel() not in (1, n):
        raise ValueError(f"overlay_render: thr must hold 1 or n = {n} values, got {tuple(thr.shape)}")
    if (count is None) != (ints is None):
        raise ValueError("overlay_render: count and ints come together")
    K = 1 if count is None else _chk_region_tables(count, ints, n, "overlay_render")
    line_px = int(line_px)
    if not 1 <= line_px <= 8:
        raise ValueError(f"overlay_render: line_px = {line_px} (1..8)")
    _on_device(dev, "overlay_render", lohi=lohi, lut=lut, alpha=alpha, thr=thr, background=background, count=count, ints=ints)
    canvas = _out(canvas, torch.uint8, (n, Ho, Wo, 3), dev, "overlay_render.canvas")
    nan_count = _out(nan_count, torch.int32, (1,), dev, "overlay_render.nan_count", zero=True)
    if n:
        _call("cmdiad_overlay_render", _p(maps), n, H, W, Ho, Wo, _p(lohi), lohi_per_image, _p(thr),
              int(thr is not None and thr.numel() == n and n > 1), _p(background), kind, *mean, *std, _p(lut), _p(alpha), _p(count),
              _p(ints), K, line_px, _rgb_word(contour_rgb, "overlay_render.contour_rgb"), _rgb_word(box_rgb, "overlay_render.box_rgb"),
              _p(canvas), _p(nan_count), _stream())
    else:
        nan_count.zero_()
    return canvas, nan_count


def png_filter(images_u8, mode="adaptive", out=None):
    """images [n,H,W,C] uint8 (C in 1..4; [n,H,W] is one channel) -> scanlines [n, H * (1 + W * C)] uint8: every row its filter byte
    and its filtered bytes, what utils.png.encode deflates and cmdiad_png_unfilter undoes.  mode: one of PNG_FILTER_MODES or its
    index; 'adaptive' picks per row the type with the smallest sum of min(b, 256 - b).  No synchronisation."""
    _chk(images_u8, torch.uint8, "png_filter.images")
    if images_u8.dim() == 3:
        images_u8 = images_u8.unsqueeze(-1)
    if images_u8.dim() != 4:
        raise ValueError(f"png_filter: images must be [n,H,W,C] or [n,H,W], got {tuple(images_u8.shape)}")
    refusal = f"png_filter: unsupported shape {tuple(images_u8.shape)} (n <= {FRAME_MAX_IMAGES}, sides 1..2^14, C in 1..4)"
    n, H, W = _frames(images_u8.shape[:3], "png_filter", side=FRAME_MAX_SIDE, pixels=None, total=None, msg=refusal)
    C = images_u8.shape[3]
    if not 1 <= C <= 4:
        raise ValueError(refusal)
    if isinstance(mode, str):
        if mode not in PNG_FILTER_MODES:
            raise ValueError(f"png_filter: mode must be one of {PNG_FILTER_MODES}, got {mode!r}")
        mode = PNG_FILTER_MODES.index(mode)
    mode = int(mode)
    if not 0 <= mode <= 5:
        raise ValueError(f"png_filter: mode = {mode} (0..5)")
    out = _out(out, torch.uint8, (n, H * (1 + W * C)), images_u8.device, "png_filter.out")
    if n:
        _call("cmdiad_png_filter", _p(images_u8), n, H, W, C, mode, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------ meshes (docs/mesh.md)
MESH_CHUNK = 1024                 # pixels per entry of cmdiad_mesh_count's chunks table
MESH_VERTEX_BYTES, MESH_FACE_BYTES = 35, 13


def _mesh_geometry(cloud, maps, max_edge2, layout, who):
    """the checks mesh_count and mesh_write share -> (n, H, W, planar, max_edge2)"""
    n, H, W = _chk_maps(maps, who)
    _chk(cloud, torch.float32, f"{who}.cloud")
    _frames(maps.shape, who, side=FRAME_MAX_SIDE, total=MESH_MAX_TOTAL, msg=f"{who}: maps {tuple(maps.shape)}: sides 1..2^14, n*H*W <= 2^24")
    planar = cloud_layout(cloud, H, W, layout, who) == "planar"
    if cloud.shape[0] != n or cloud.device != maps.device:
        raise ValueError(f"{who}: {cloud.shape[0]} clouds on {cloud.device} for {n} maps on {maps.device}")
    max_edge2 = float(max_edge2)
    if not max_edge2 > 0:
        raise ValueError(f"{who}: max_edge2 = {max_edge2!r} must be > 0 (inf: no edge is cut)")
    return n, H, W, planar, max_edge2


def mesh_count(cloud, maps, max_edge2=float("inf"), out=None, layout=None):
    """The organised cloud of the maps (f32, planar [n,3,H,W] or interleaved [n,H,W,3], worked out from the shape; layout= where H or
    W is 3) and maps [n,H,W] f64 -> (chunks [n,C,2] i32 = vertices and faces per run of MESH_CHUNK pixels, C = ceil(H W / MESH_CHUNK);
    counts [n,4] i32 = n_vert, n_face, bad, nan).  out: that pair, to write into.  docs/mesh.md has the contract.  No
    synchronisation."""
    n, H, W, planar, max_edge2 = _mesh_geometry(cloud, maps, max_edge2, layout, "mesh_count")
    dev, C = maps.device, -(-H * W // MESH_CHUNK)
    chunks, counts = out or (None, None)
    chunks = _out(chunks, torch.int32, (n, C, 2), dev, "mesh_count.chunks")
    counts = _out(counts, torch.int32, (n, 4), dev, "mesh_count.counts")
    if n:
        _call("cmdiad_mesh_count", _p(cloud), 1 if planar else 3, H * W if planar else 1, _p(maps), n, H, W, max_edge2, _p(chunks),
              _p(counts), _stream())
    return chunks, counts


def mesh_write(cloud, maps, chunks, lohi, lut, alpha, background=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), labels=None,
               max_edge2=float("inf"), flip=False, out=None, layout=None):
    """cloud, maps and chunks as mesh_count takes and leaves them (the same max_edge2) -> (vidx [n,H,W] i32, vertices [n, H W 35] u8,
    faces [n, 2 (H-1) (W-1) 13] u8): image i fills the front of its rows with its counts[i,0] vertex and counts[i,1] face records.
    lohi ([2] or [n,2] f64), lut [256,3] u8, alpha [256] u8, background (None, uint8 [n,H,W,3] or float32 [n,3,H,W] with mean / std)
    as overlay_render takes them; labels [n,H,W] i32 or None (region 0).  out: that triple, to write into.  No synchronisation."""
    n, H, W, planar, max_edge2 = _mesh_geometry(cloud, maps, max_edge2, layout, "mesh_write")
    dev, C = maps.device, -(-H * W // MESH_CHUNK)
    _chk(chunks, torch.int32, "mesh_write.chunks"); _chk(labels, torch.int32, "mesh_write.labels")
    if chunks is None:
        raise ValueError("mesh_write: chunks, lohi, lut and alpha are required")
    if tuple(chunks.shape) != (n, C, 2):
        raise ValueError(f"mesh_write: chunks must be [{n},{C},2] (mesh_count's), got {tuple(chunks.shape)}")
    kind, lohi_per_image, mean, std = _chk_colours("mesh_write", n, H, W, lohi, lut, alpha, background, mean, std)
    if labels is not None and labels.shape != maps.shape:
        raise ValueError(f"mesh_write: labels must have the maps' shape {tuple(maps.shape)}, got {tuple(labels.shape)}")
    _on_device(dev, "mesh_write", chunks=chunks, lohi=lohi, lut=lut, alpha=alpha, background=background, labels=labels)
    vidx, vertices, faces = out or (None, None, None)
    vidx = _out(vidx, torch.int32, (n, H, W), dev, "mesh_write.vidx")
    vertices = _out(vertices, torch.uint8, (n, H * W * MESH_VERTEX_BYTES), dev, "mesh_write.vertices")
    faces = _out(faces, torch.uint8, (n, 2 * (H - 1) * (W - 1) * MESH_FACE_BYTES), dev, "mesh_write.faces")
    if n:
        _call("cmdiad_mesh_write", _p(cloud), 1 if planar else 3, H * W if planar else 1, _p(maps), n, H, W, _p(lohi),
              lohi_per_image, _p(lut), _p(alpha), _p(background), kind, *mean, *std, _p(labels), max_edge2,
              int(bool(flip)), _p(chunks), _p(vidx), _p(vertices), _p(faces) if faces.numel() else None, _stream())
    return vidx, vertices, faces


# ------------------------------------------------------------------------------------ point lists into the pixel grid (docs/organize.md)
ORGANIZE_KEY_EMPTY = -1           # all ones, as the int64 torch shows


def _chk_point_list(points, offsets, cams, max_len, who):
    """the checks the three entry points share -> (n, P, max_len)"""
    _chk(points, torch.float32, f"{who}.points"); _chk(offsets, torch.int64, f"{who}.offsets"); _chk(cams, torch.float64, f"{who}.cams")
    if points is None or offsets is None:
        raise ValueError(f"{who}: points and offsets are required")
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError(f"{who}: points must be [P,3] and offsets [n+1], got {tuple(points.shape)} and {tuple(offsets.shape)}")
    n, P = offsets.numel() - 1, points.shape[0]
    if n > FRAME_MAX_IMAGES or P >= 1 << 31:
        raise ValueError(f"{who}: {n} clouds (at most {FRAME_MAX_IMAGES}) of {P} points (below 2^31)")
    if offsets.device != points.device:
        raise ValueError(f"{who}: offsets on {offsets.device}, points on {points.device}")
    if cams is not None and (tuple(cams.shape) != (n, 16) or cams.device != points.device):
        raise ValueError(f"{who}: cams must be [{n},16] float64 on the points' device, got {tuple(cams.shape)} on {cams.device}")
    max_len = int(max_len)
    if not 0 <= max_len < 1 << 31:
        raise ValueError(f"{who}: max_len = {max_len} (0..2^31-1)")
    return n, P, max_len


def _chk_grid(n, H, W, who):
    return _frames((n, H, W), who, msg=f"{who}: a grid of {int(H)} x {int(W)} for {n} clouds: sides >= 1, H*W <= 2^24, n*H*W <= 2^30")[1:]


def cloud_bounds(points, offsets, cams, max_len, out=None):
    """points [P,3] f32, offsets [n+1] i64 (on the device), cams [n,16] f64, max_len (the longest cloud) -> (bounds [n,6] f64 = the
    minimum of the camera coordinates c_0..c_2 over each cloud's valid points, then the maximum; count [n] i32 = the valid points).
    An empty cloud gives +inf, -inf, 0.  out: that pair, to write into.  No synchronisation."""
    n, P, max_len = _chk_point_list(points, offsets, cams, max_len, "cloud_bounds")
    if cams is None:
        raise ValueError("cloud_bounds: cams is required")
    dev = points.device
    bounds, count = out or (None, None)
    bounds = _out(bounds, torch.float64, (n, 6), dev, "cloud_bounds.bounds")
    count = _out(count, torch.int32, (n,), dev, "cloud_bounds.count")
    if n:
        _call("cmdiad_cloud_bounds", _p(points), _p(offsets), _p(cams), n, P, max_len, _p(bounds), _p(count), _stream())
    return bounds, count


def organize_splat(points, offsets, cams, max_len, kind, H, W, out=None):
    """The projection and the nearest-point key map: -> (keys [n,H,W] i64 (the uint64 bits; ORGANIZE_KEY_EMPTY where no point fell),
    pixel_of_point [P] i32 (-2 dropped, -1 outside, else the pixel; written for the points of the clouds only), stats [n,4] i32
    with columns 0, 1 = dropped, outside).  kind: 0 orthographic, 1 pinhole.  out: that triple, to write into (a fresh stats is
    zeroed; a given one keeps its columns 2, 3).  No synchronisation."""
    n, P, max_len = _chk_point_list(points, offsets, cams, max_len, "organize_splat")
    if cams is None:
        raise ValueError("organize_splat: cams is required")
    H, W = _chk_grid(n, H, W, "organize_splat")
    kind = int(kind)
    if kind not in (0, 1):
        raise ValueError(f"organize_splat: kind = {kind} (0 orthographic | 1 pinhole)")
    dev = points.device
    keys, pixel_of_point, stats = out or (None, None, None)
    keys = _out(keys, torch.int64, (n, H, W), dev, "organize_splat.keys")
    pixel_of_point = _out(pixel_of_point, torch.int32, (P,), dev, "organize_splat.pixel_of_point")
    stats = _out(stats, torch.int32, (n, 4), dev, "organize_splat.stats", zero=True)
    if n:
        _call("cmdiad_organize_splat", _p(points), _p(offsets), _p(cams), n, P, max_len, kind, H, W, _p(keys), _p(pixel_of_point),
              _p(stats), _stream())
    return keys, pixel_of_point, stats


def organize_resolve(points, offsets, keys, stats, fill=0, colors=None, labels=None, want_rgb=True, want_mask=True, out=None):
    """The key map of organize_splat -> (index [n,H,W] i32, xyz [n,H,W,3] f32, rgb [n,H,W,3] u8 | None, mask [n,H,W] u8 | None); stats
    columns 2, 3 = direct, filled pixels.  colors [P,3] u8 and labels [P] u8 are optional (absent: zeros); fill in 0..2.  out: that
    quadruple, to write into (None in the place of an output that is not wanted).  No synchronisation."""
    n, P, _ = _chk_point_list(points, offsets, None, 0, "organize_resolve")
    _chk(keys, torch.int64, "organize_resolve.keys"); _chk(colors, torch.uint8, "organize_resolve.colors")
    _chk(labels, torch.uint8, "organize_resolve.labels")
    if keys is None or keys.dim() != 3 or keys.shape[0] != n:
        raise ValueError(f"organize_resolve: keys must be [{n},H,W] int64")
    H, W = _chk_grid(n, keys.shape[1], keys.shape[2], "organize_resolve")
    fill = int(fill)
    if fill not in (0, 1, 2):
        raise ValueError(f"organize_resolve: fill = {fill} (0..2)")
    dev = points.device
    if colors is not None and (tuple(colors.shape) != (P, 3) or colors.device != dev):
        raise ValueError(f"organize_resolve: colors must be [{P},3] uint8 on the points' device, got {tuple(colors.shape)}")
    if labels is not None and (tuple(labels.shape) != (P,) or labels.device != dev):
        raise ValueError(f"organize_resolve: labels must be [{P}] uint8 on the points' device, got {tuple(labels.shape)}")
    if keys.device != dev:
        raise ValueError("organize_resolve: keys must be on the points' device")
    _chk_out(stats, torch.int32, (n, 4), dev, "organize_resolve.stats")
    if out is None:
        out = (torch.empty((n, H, W), dtype=torch.int32, device=dev), torch.empty((n, H, W, 3), dtype=torch.float32, device=dev),
               torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev) if want_rgb else None,
               torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_mask else None)
    index, xyz, rgb, mask = out
    _chk_out(index, torch.int32, (n, H, W), dev, "organize_resolve.index")
    _chk_out(xyz, torch.float32, (n, H, W, 3), dev, "organize_resolve.xyz")
    if rgb is not None:
        _chk_out(rgb, torch.uint8, (n, H, W, 3), dev, "organize_resolve.rgb")
    if mask is not None:
        _chk_out(mask, torch.uint8, (n, H, W), dev, "organize_resolve.mask")
    if n:
        _call("cmdiad_organize_resolve", _p(points), _p(offsets), _p(colors), _p(labels), _p(keys), n, P, H, W, fill, _p(index),
              _p(xyz), _p(rgb), _p(mask), _p(stats), _stream())
    return index, xyz, rgb, mask


# ------------------------------------------------------------------------------------ content digest (stored fits)
def digest64(tensor, seed=0, acc=None):
    """cmdiad_digest64 of a device tensor's bytes, ADDED into `acc` ([1] int64 on the tensor's device; None: a fresh zero) -> acc.
    The tensor must be contiguous and a multiple of 4 bytes long (module_digest pads the others); `seed` is taken mod 2^64.
    Nothing is read back: `digest_value(acc)` is the one device-to-host copy.  (include/cmdiad_hip.h has the definition.)"""
    if not tensor.is_cuda:
        raise nat.NativeError("digest64: tensor must live on the GPU (the host restatement is fitted.digest64_host)")
    if not tensor.is_contiguous():
        raise ValueError("digest64: tensor must be contiguous")
    nbytes = tensor.numel() * tensor.element_size()
    if nbytes % 4:
        raise ValueError(f"digest64: {nbytes} bytes is not a multiple of 4")
    if acc is None:
        acc = torch.zeros((1,), dtype=torch.int64, device=tensor.device)
    elif not (acc.is_cuda and acc.dtype == torch.int64 and acc.numel() == 1 and acc.device == tensor.device):
        raise ValueError("digest64: acc must be one int64 on the tensor's device")
    _call("cmdiad_digest64", _p(tensor), nbytes, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(acc), _stream())
    return acc


def digest_value(acc):
    """The accumulator of digest64 as a Python int in [0, 2^64) (one device-to-host read)."""
    return int(acc.item()) & 0xFFFFFFFFFFFFFFFF


def tensor_seed(key, tensor):
    """Seed of a named tensor in module_digest: the first 8 bytes (little-endian) of sha256("<key>|<dtype>|<shape>"), e.g.
    "blocks.0.attn.qkv.weight|torch.float32|(2304, 768)" -- a renamed, re-typed or re-shaped tensor changes the digest."""
    import hashlib
    text = f"{key}|{tensor.dtype}|{tuple(tensor.shape)}"
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")


def module_digest(module, device=None):
    """Digest of every tensor of `module.state_dict()` (key order), each seeded by tensor_seed, all added into ONE device
    accumulator: one device-to-host read for the whole module, no copy of the weights.  A tensor whose byte size is no multiple
    of 4 is hashed from a zero-padded device copy; a tensor that is not on the GPU is copied there first."""
    sd = module.state_dict()
    acc = None
    for key in sorted(sd):
        t = sd[key].detach()
        if not t.is_cuda:
            t = t.to(device or "cuda")
        raw = t.contiguous().reshape(-1).view(torch.uint8)
        if raw.numel() % 4:
            raw = torch.cat([raw, raw.new_zeros(4 - raw.numel() % 4)])
        if acc is None:
            acc = torch.zeros((1,), dtype=torch.int64, device=raw.device)
        digest64(raw, tensor_seed(key, sd[key]), acc)
    return digest_value(acc) if acc is not None else 0
