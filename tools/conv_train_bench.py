#!/usr/bin/env python3
"""Training step of the convolutional FtoF head (HallucinationCrossModalityConv, both directions: forward, loss, backward, Adam):
the hand-written path (cmdiad_amd/conv_train.py) against the module's own torch layers (tests/heads_torch_ref.py).
    python tools/conv_train_bench.py [batch] [steps] [hip|torch: one side only]"""
import os, sys, time, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import heads_torch_ref as torch_ref
from cmdiad_amd.models import hallucination_network as hn
from oracle import heads
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
modes = (sys.argv[3],) if len(sys.argv) > 3 else ("hip", "torch")
gen = torch.Generator().manual_seed(1)
a, b = torch.randn(B, 3136, 768, generator=gen).cuda(), torch.randn(B, 3136, 768, generator=gen).cuda()
flop = 2 * 4 * 3 * 2.0 * B * 3136 * 768 * 9 * 768 - 2 * 2.0 * B * 3136 * 768 * 9 * 768   # 2 towers x 4 convs x (fwd, dgrad, wgrad), no dgrad for the first
img = torch.randn(B, 3, 224, 224, generator=gen).cuda()
for kind, make, ref, x in (("ftoi_conv", lambda: hn.HallucinationFeatureToInputConv(None, 768), torch_ref.ftoi_conv_loss, (a, img)),
                           ("hrnet", lambda: __import__("cmdiad_amd.models.hrnet", fromlist=["HRNet"]).HRNet(512, 768, 0.1), torch_ref.hrnet_loss, (img, a)),
                           ("ftoi_mlp", lambda: hn.HallucinationRGBFeatureToXYZInputMLP(__import__("types").SimpleNamespace(estimate_depth=False), 768), torch_ref.ftoi_mlp_loss, (a, img))):
    for mode in modes:
        m = make(); m.load_state_dict(heads.synth_head_state_dict(kind, 41)); m.cuda().train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        def step():
            opt.zero_grad(); loss = m(*x) if mode == "hip" else ref(m, *x); loss.backward(); opt.step(); return float(loss.detach())
        step(); step(); torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps): last = step()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
        print(f"{kind} head training step, batch {B}, {mode}: {dt * 1e3:.1f} ms (loss {last:.2f}), peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
        del m, opt; torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
for mode in modes:
    m = hn.HallucinationCrossModalityConv(None, 768, 768)
    m.load_state_dict(heads.synth_head_state_dict("conv_ftof", 41))
    m.cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    def step():
        opt.zero_grad()
        lx, lr = m(a, b, False, "l2") if mode == "hip" else torch_ref.conv_ftof_losses(m, a, b, False)
        (lx + lr).backward()
        opt.step()
        return float(lx.detach())
    step(); step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): last = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    print(f"conv head training step, batch {B}, {mode}: {dt * 1e3:.1f} ms = {flop / dt / 1e12:.0f} TFLOP/s (loss {last:.4f}), "
          f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    del m, opt; torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
