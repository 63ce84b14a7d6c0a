#!/usr/bin/env python
"""The res3 block-pair kernel alone against the two launches it replaces, on the R-50 res3 shape (100 x 168, 512 / 128 channels):
conv_spw_kernel_pair vs conv_spw_kernel (conv3 + residual) + conv_igemm_kernel (the next block's conv1).  Kernel times are HIP events
around the launches (Engine.profile_read); TB/s on the bytes each form has to move (pair: t2 + x in, y + t1 out).
Usage (GPU box): python tools/bench_res3_pair.py [batch = 64] [iters = 5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))
from sylph_amd.engine import Engine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
IT = int(sys.argv[2]) if len(sys.argv) > 2 else 5
H, W = 100, 168
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
t2 = torch.relu(torch.randn(B, 128, H, W, device=dev, generator=g))
x = torch.relu(torch.randn(B, 512, H, W, device=dev, generator=g))
w3 = torch.randn(512, 128, 1, 1) * (2.0 / 128) ** 0.5
w1 = torch.randn(128, 512, 1, 1) * (2.0 / 512) ** 0.5
s3, b3, s1, b1 = torch.rand(512) + 0.5, torch.randn(512) * 0.2, torch.rand(128) + 0.5, torch.randn(128) * 0.2
eng = Engine(None, dtype="bf16")
rows = B * H * W
eng.res3_pair(t2, x, w3, s3, b3, w1, s1, b1)  # warm-up
y = eng.conv2d(t2, w3, s3, b3, relu=True, residual=x)
eng.conv2d(y, w1, s1, b1, relu=True)
eng.profile_enable(True)
eng.profile_read()
for _ in range(IT):
    eng.res3_pair(t2, x, w3, s3, b3, w1, s1, b1)
kp = eng.profile_read()["kernels"]
for _ in range(IT):
    y = eng.conv2d(t2, w3, s3, b3, relu=True, residual=x)
k3 = eng.profile_read()["kernels"]
for _ in range(IT):
    eng.conv2d(y, w1, s1, b1, relu=True)
k1 = eng.profile_read()["kernels"]
eng.profile_enable(False)


def line(name, k, byts):
    (kn, v), = k.items()
    ms = v["ms"] / v["launches"]
    print(f"{name:28s} {kn:24s} {ms * 1e3:8.1f} us  {byts / (ms * 1e-3) / 1e12:5.2f} TB/s on {byts / 1e9:.2f} GB")
    return ms


mp = line("pair (one launch)", kp, rows * (128 + 512 + 512 + 128) * 2)
m3 = line("conv3 + residual", k3, rows * (128 + 512 + 512) * 2)
m1 = line("next conv1", k1, rows * (512 + 128) * 2)
print(f"batch {B}: pair {mp * 1e3:.1f} us vs {(m3 + m1) * 1e3:.1f} us for the two launches ({(m3 + m1) / mp:.3f} x)")
