"""Worker of tests/test_gpu_attention_edges.py: cmdiad_gemm_qkv reads CMDIAD_QKV_VROWS once per process, so the direct V^T store
form (CMDIAD_QKV_VROWS=0) needs a process of its own.  Runs the with-bias form of every case of attn_ref.QKV_GRID on the exact
operands and saves the three buffers, padding included, for the parent to compare with the default form and the reference.
Launched as: CMDIAD_QKV_VROWS=0 python tests/qkv_vrows_worker.py OUT.pt"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import attn_ref as ar  # noqa: E402
from cmdiad_amd import ops  # noqa: E402


def main():
    assert os.environ.get("CMDIAD_QKV_VROWS") == "0"
    out = {}
    for B, T, C in ar.QKV_GRID:
        A, W, bias, _ = ar.qkv_exact_operands(B, T, C)
        q, k, vt = ar.qkv_filled_buffers(B, C // 64, T, "cuda")
        ops.gemm_qkv(A.cuda(), W.cuda(), bias.cuda(), B, T, q, k, vt)
        out[(B, T, C)] = (q.cpu(), k.cpu(), vt.cpu())
    torch.save(out, sys.argv[1])
    print(f"qkv_vrows_worker: {len(out)} cases")


if __name__ == "__main__":
    main()
