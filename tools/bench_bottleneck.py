#!/usr/bin/env python
"""Micro-benchmark of one identity bottleneck block at its production shape (default: res2, B x 200 x 336, C 256, mid 64: the fused
bottleneck.hip kernel; stage 3 / 4 / 5: the three conv launches of a res3 / res4 / res5 identity block).
HIP-event time of the kernel launch alone (sylph_profile), so the layout conversions of the parity entry are not in it.
Usage (GPU box): [SYLPH_LIB_PATH=<another build of the library>] python tools/bench_bottleneck.py [batch] [iters] [stage] [even]
`even` (stage 2 only): also time the stride-2-output launch of the same block (the last block of res2 in the backbone: outputs at the even
rows / columns only, bottleneck64_kernel<3, 1, 2, false, true>) on the same input, after the dense one.
(the ablation builds it was used with, tools/build_variant.sh, are in git history at ac4cfc5)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))
from sylph_amd.engine import Engine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 6
stage = int(sys.argv[3]) if len(sys.argv) > 3 else 2
even = len(sys.argv) > 4 and sys.argv[4] == "even"
if even and stage != 2:
    sys.exit("even: the stride-2-output launch exists for the res2 block only")
mid, C, Hm, Wm = 64 << (stage - 2), 256 << (stage - 2), 200 >> (stage - 2), 336 >> (stage - 2)
g = torch.Generator().manual_seed(0)
eng = Engine(None, dtype="bf16")
x = torch.randn(B, C, Hm, Wm, generator=g).cuda()
ws = [torch.randn(mid, C, 1, 1, generator=g) / C ** 0.5, torch.randn(mid, mid, 3, 3, generator=g) / (9 * mid) ** 0.5,
      torch.randn(C, mid, 1, 1, generator=g) / mid ** 0.5]
sc = [torch.rand(mid, generator=g) + 0.5, torch.rand(mid, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5]
sh = [torch.randn(mid, generator=g) * 0.1, torch.randn(mid, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1]
eng.bottleneck(x, ws, sc, sh, 1)
eng.profile_enable(True)
for _ in range(iters):
    eng.bottleneck(x, ws, sc, sh, 1)
torch.cuda.synchronize()


def report(tag, bytes_per_pos, what):
    for name, k in eng.profile_read()["kernels"].items():
        ms, fl, n = k["ms"], k["flops"], max(k["launches"], 1)
        pos = B * Hm * Wm
        print(f"{os.environ.get('SYLPH_LIB_PATH', 'product')[-40:]:40s} {name + tag:28s} {ms / n * 1e3:8.1f} us/launch  "
              f"{fl / (ms * 1e-3) / 1e12:7.1f} TFLOP/s  {pos * bytes_per_pos / (ms / n * 1e-3) / 1e12:5.2f} TB/s (at {what} / position)")


report("", 1024, "1 KiB")
if even:
    eng.profile_enable(False)
    eng.bottleneck_even(x, ws, sc, sh)
    eng.profile_enable(True)
    eng.profile_read()
    for _ in range(iters):
        eng.bottleneck_even(x, ws, sc, sh)
    torch.cuda.synchronize()
    report(" (even)", 640, "512 B in + 128 B out")
