"""SHA-256 of every output tensor of the three training gradients on fixed, seeded cases whose partial sums span several levels of
the reduction tree (csrc/partial_sum.h).  Two builds that print the same lines compute the same bits; nothing here is a tolerance.

  cls_grad      40 images of 128 x 160, 5 classes: 70 units, two levels at fan-in 64 (tests/test_finetune_gpu.py)
  box_grad      3 images of 256 x 320 with 40 boxes each, the bank tiled to >= 5000 samples: 168 units, two levels at fan-in 64
  codegen       a depth-1 generator, 257 shots over a 12-row bank in 4 segments: 65 units, three levels at fan-in 8; forward + backward

One process, one JSON line per tensor.  Needs a GPU.
    python tools/train_grad_digest.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sylph-few-shot-detection_amd"))

import torch  # noqa: E402


def digest(case, name, t):
    t = t.detach().cpu().contiguous()
    print(json.dumps({"case": case, "tensor": name, "shape": list(t.shape), "sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest()}), flush=True)


def cfg(depth):
    from sylph_amd.config import get_default_cfg
    c = get_default_cfg()
    cg = c.MODEL.META_LEARN.CODE_GENERATOR
    c.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.POST_NORM = "GN"
    cg.TOWER_LAYERS = [["GN", "ReLU"]] * depth
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    return c


def pyramid(eng, B, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 256, h, w, generator=g).to(torch.bfloat16).float() for h, w in eng.level_shapes(*hw)]


def boxes(n_images, per_image, hw, n_classes, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    n = n_images * per_image
    bw, bh = lo + torch.rand(n, generator=g) * (hi - lo), lo + torch.rand(n, generator=g) * (hi - lo)
    x0, y0 = torch.rand(n, generator=g) * (hw[1] - bw), torch.rand(n, generator=g) * (hw[0] - bh)
    return torch.stack([x0, y0, x0 + bw, y0 + bh], 1), torch.randint(0, n_classes, (n,), generator=g), torch.arange(n_images).repeat_interleave(per_image)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("train_grad_digest.py needs a GPU")
    from sylph_amd import synthetic as W
    from sylph_amd.engine import BoxSamples, Engine

    eng = Engine(cfg(2), dtype="bf16")
    eng.load_state_dict(W.head_state_dict(seed=3))
    # cls_grad: 40 x 428 rows = 280 tiles = 70 units
    hw = (128, 160)
    eng.import_pyramid(pyramid(eng, 40, hw, seed=12), hw)
    eng.towers()
    rows = eng.batch_rows()
    g = torch.Generator().manual_seed(13)
    lab = torch.where(torch.rand(rows, generator=g) < 0.05, torch.randint(0, 5, (rows,), generator=g), torch.tensor(-1)).to(torch.int32)
    codes = W.synthetic_codes(5, seed=105, scale=2.5)
    loss, gw, gb = eng.cls_grad(lab.cuda(), codes["cls_conv"].cuda(), codes["cls_bias"].cuda())
    for name, t in (("loss", loss), ("grad_w", gw), ("grad_b", gb)):
        digest("cls_grad", name, t)
    # box_grad: the bank of a 3-image batch, tiled
    hw = (256, 320)
    eng.import_pyramid(pyramid(eng, 3, hw, seed=8), hw)
    eng.towers()
    bank = eng.box_samples(*boxes(3, 40, hw, 20, seed=9, lo=4.0, hi=300.0))
    bank = BoxSamples.cat([bank] * ((5000 + bank.n - 1) // bank.n))
    assert (bank.n + 31) // 32 > 64, bank.n
    br = eng.box_branch()
    from sylph_amd.finetune import stack_box_branch
    out = eng.box_grad(bank, *stack_box_branch(br), debug=True, quality=["ctrness", "iou"], iou_mask=False)
    digest("box_grad", "samples", torch.tensor([bank.n]))
    for name in ("sums", "grad_w", "grad_b", "grad_scales", "z", "g"):
        digest("box_grad", name, out[name])
    eng.close()

    # codegen forward + backward: 257 shots in 65 units -> 9 -> 2 -> the final pass
    eng = Engine(cfg(1), dtype="bf16")
    eng.load_state_dict(W.codegen_state_dict(seed=2, tower_layers=1))
    M, seg_len = 257, [64, 64, 64, 65]
    shp = eng.codegen_train_shape(M, len(seg_len))
    assert shp["units"] == 65 and shp["passes"] == 3, shp
    g = torch.Generator().manual_seed(257)
    bank_rows = (torch.rand(12, 49, 256, generator=g) * 2.0).to(torch.bfloat16).cuda()
    flat = eng.code_generator().cuda()
    codes = eng.codegen_train_forward(flat, bank_rows, [(7 * i) % 12 for i in range(M)], seg_len)
    G = torch.randn(len(seg_len), 257, generator=torch.Generator().manual_seed(8)).cuda()
    grad = eng.codegen_train_backward(G)
    digest("codegen", "codes", codes)
    digest("codegen", "grad", grad)
    for k, o, n in eng.codegen_params():
        digest("codegen", "grad:" + k.split("head.")[-1], grad[o:o + n])
    eng.close()


if __name__ == "__main__":
    main()
