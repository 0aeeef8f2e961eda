#!/usr/bin/env python3
"""Same-box A/B of the two-group 256 x 256 network GEMMs (gemm_pp3.h: persistent, persistent + row_scale, stream-K, one tile per
block) between two builds of the library, e.g. the committed one against a side build of its parent commit:
    git archive <commit> cmdiad_amd/csrc include | tar -x -C /tmp/old && make -C /tmp/old/cmdiad_amd/csrc OUT=$PWD/cmdiad_amd/libcmdiad_hip_parent.so
    python tools/two_group_ab.py [old.so [new.so [passes]]]
Both libraries are loaded through ctypes into ONE process.  Per shape: the outputs on seeded inputs must be torch.equal; then the
two alternate for `passes` (>= 5) passes of 8 launches with HIP events around every launch (first two dropped, median of the
rest = the pass median).  The margin is the OLD build's own pass-to-pass spread (max - min of its pass medians): the new
build's median over the passes may exceed the old build's slowest pass by that much, else the exit code is 1."""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdiad_amd import _native as nat  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmdiad_amd")
paths = {"old": sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "libcmdiad_hip_parent.so"),
         "new": sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "libcmdiad_hip.so")}
passes = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
P = ctypes.c_void_p
libs = {}
for tag, path in paths.items():
    L = ctypes.CDLL(path)
    L.cmdiad_gemm_bf16.argtypes = [ctypes.POINTER(nat.GemmArgs), P]
    L.cmdiad_gemm_streamk_bf16.argtypes = [ctypes.POINTER(nat.GemmArgs), P, ctypes.c_size_t, P]
    L.cmdiad_gemm_streamk_workspace_bytes.restype = ctypes.c_size_t
    L.cmdiad_last_error.restype = ctypes.c_char_p
    assert L.cmdiad_abi_version() == libs.get("old", L).cmdiad_abi_version(), "the two builds differ in ABI"
    libs[tag] = L

ACT_NONE, ACT_GELU = 0, 1
# (name, M, N, K, form, environment of the launch)
CASES = [("persistent fc1 + GELU", 25120, 3072, 768, "bf16", {"CMDIAD_GEMM_PP3": "1"}),
         ("persistent + row_scale + GELU", 32768, 1536, 384, "row_scale", {"CMDIAD_GEMM_PP3": "1"}),
         ("stream-K fc2", 25120, 768, 3072, "streamk", {}),
         ("one tile per block (CMDIAD_GEMM_RES_WIDE=1)", 25120, 768, 768, "residual", {"CMDIAD_GEMM_RES_WIDE": "1"})]
SWITCHES = ("CMDIAD_GEMM_PP3", "CMDIAD_GEMM_RES_WIDE")
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
ws = {tag: torch.zeros((L.cmdiad_gemm_streamk_workspace_bytes(),), dtype=torch.uint8, device=dev) for tag, L in libs.items()}
failed = False
for name, M, N, K, form, env in CASES:
    A = torch.randn(M, K, generator=g).to(dev).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).bfloat16()
    bias = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev) if form in ("streamk", "residual") else None
    rsc = (torch.rand((M + 255) // 256 * 256, generator=g) + 0.5).to(dev) if form == "row_scale" else None
    o16 = torch.empty((M, N), dtype=torch.bfloat16, device=dev) if res is None else None
    o32 = torch.empty((M, N), dtype=torch.float32, device=dev) if res is not None else None
    a = nat.GemmArgs(p(A), K, p(W), K, M, N, K, p(bias), None, 1, ACT_GELU if res is None else ACT_NONE,
                     p(res), N, p(o32), N, p(o16), N, None, None, 1, None, p(rsc), None, N, None, None, N)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for s in SWITCHES:
        os.environ.pop(s, None)
    os.environ.update(env)

    def launch(tag):
        L = libs[tag]
        rc = (L.cmdiad_gemm_streamk_bf16(ctypes.byref(a), p(ws[tag]), ws[tag].numel(), st) if form == "streamk"
              else L.cmdiad_gemm_bf16(ctypes.byref(a), st))
        assert rc == 0, (tag, name, L.cmdiad_last_error())

    out = o16 if o16 is not None else o32
    got = {}
    for tag in libs:
        out.zero_()
        launch(tag)
        torch.cuda.synchronize()
        got[tag] = out.clone()
    same = torch.equal(got["old"], got["new"])
    print(f"{name} {M} x {N} x {K}: outputs {'identical' if same else 'DIFFER'}", flush=True)
    failed |= not same
    med = {tag: [] for tag in libs}
    for ps in range(passes):
        for tag in libs:
            ts = []
            for it in range(8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(tag)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            med[tag].append(statistics.median(ts[2:]))
        print(f"  pass {ps}: old {med['old'][-1]:.1f} us   new {med['new'][-1]:.1f} us", flush=True)
    spread = max(med["old"]) - min(med["old"])
    new_med, limit = statistics.median(med["new"]), max(med["old"]) + spread
    ok = new_med <= limit
    print(f"  old pass medians {min(med['old']):.1f} .. {max(med['old']):.1f} us (spread {spread:.1f}), median {statistics.median(med['old']):.1f};"
          f"  new median {new_med:.1f} us ({2.0 * M * N * K / new_med / 1e6:.0f} TFLOP/s), limit {limit:.1f}: {'ok' if ok else 'SLOWER'}", flush=True)
    failed |= not ok
sys.exit(1 if failed else 0)
