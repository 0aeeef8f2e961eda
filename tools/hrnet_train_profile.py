#!/usr/bin/env python3
"""HRNet head training steps alone (for a kernel trace): rocprofv3 --kernel-trace --stats -- python3 tools/hrnet_train_profile.py [batch] [hip|torch]
(hip: the hand-written path, the default; torch: the module's own torch layers, tests/heads_torch_ref.py)"""
import os, sys, time, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import heads_torch_ref as torch_ref
from cmdiad_amd.models.hrnet import HRNet
from oracle import heads
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mode = sys.argv[2] if len(sys.argv) > 2 else "hip"
gen = torch.Generator().manual_seed(1)
img, feat = torch.randn(B, 3, 224, 224, generator=gen).cuda(), torch.randn(B, 3136, 768, generator=gen).cuda()
m = HRNet(512, 768, 0.1); m.load_state_dict(heads.synth_head_state_dict("hrnet", 41)); m.cuda().train()
opt = torch.optim.Adam(m.parameters(), lr=1e-4)
def step():
    opt.zero_grad(); loss = m(img, feat) if mode == "hip" else torch_ref.hrnet_loss(m, img, feat); loss.backward(); opt.step(); return loss
W, K = int(os.environ.get("WARM", "1")), int(os.environ.get("STEPS", "3"))   # (the first steps grow the caching allocator: WARM=5 for timings)
for _ in range(W): step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(K): step()
torch.cuda.synchronize(); print(f"hrnet training step, batch {B}, {mode}: {(time.perf_counter() - t0) / K * 1e3:.1f} ms")
