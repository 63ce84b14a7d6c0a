"""MODEL.FCOS.USE_DEFORMABLE on the GPU (csrc/conv_deform.hip through the C ABI), pinned to tests/deform_ref.py.

  * layer pin (bf16): the deformable layer's conv output of both towers over a full 800 x 1344 pyramid, B = 2, on the input the
    HIP graph itself produced (layer n-2 after its GroupNorm + ReLU), against the bf16 restatement (bars in _pin_layer: the GPU's
    offset conv sums in fp32, the restatement's in float64, so an A element lands on the other side of a bf16 rounding midpoint
    now and then);
  * borders: exact constant offsets that push taps off the map on all four sides at every level (P7 = 7 x 11 included): within
    1 bf16 ulp of the restatement, i.e. the samples read zeros, never rows of the next level or image;
  * degenerate case: zero offsets and a saturated mask equal the plain-conv tower built from the same conv weights;
  * f32 / f32s: head outputs within 1e-3 of the float64 restatement, and the decoder picks the same candidates from both;
  * batch position: bf16 outputs of an image are bit-identical at B = 1, 8 and 192 (copies);
  * end to end: the episodic model and the base detector run a deformable checkpoint through the config key alone and agree.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import deform_ref as DR

pytestmark = pytest.mark.gpu

H, W = 800, 1344
LEVELS = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
P = "proposal_generator.fcos_head"
K_LAST = 9


def _cfg(deformable=True):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    cfg.MODEL.FCOS.USE_DEFORMABLE = deformable
    return cfg


def _assert_ulps(got, want, what, max_ulp=2.0, max_frac=0.05, floor=None):
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (got - want).abs()
    fl = 1e-3 * float(want.abs().max()) if floor is None else floor
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl))
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    frac, worst = float((diff > 0).float().mean()), float((diff / ulp).max())
    print(f"{what}: {frac * 100:.3f} % of elements differ, worst {worst:.2f} bf16 ulp")
    assert worst <= max_ulp and frac <= max_frac, f"{what}: {frac:.4f} of elements differ, worst {worst:.2f} ulp"
    return worst


def _ulps(got, want, fl):
    got, want = got.float().cpu(), want.float().cpu()
    mag = torch.maximum(torch.maximum(got.abs(), want.abs()), torch.full_like(want, fl))
    return (got - want).abs() / torch.exp2(torch.floor(torch.log2(mag)) - 7)


def _feats(B, seed, levels=LEVELS):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 256, h, w, generator=g).bfloat16().float() for h, w in levels]


def _run_bf16(sd, feats, hw=(H, W)):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    eng = Engine(_cfg(), dtype="bf16")
    eng.load_state_dict(sd)
    eng.set_debug_taps(True)
    eng.import_pyramid(feats, hw)
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    eng.head(codes["cls_conv"], codes["cls_bias"])
    return eng


def _pin_layer(eng, sd, what, exact_offsets, convs=(4, 4), norm="GN", pyramid=None, skip=()):
    """exact_offsets: the offset conv has zero weights, so its fp32 output is its bias on both sides and the restatement rounds
    exactly where the kernel does: every element within 1 ulp of the rounded restatement.  Otherwise the restatement's offsets come
    from a float64 offset conv and the kernel's from an fp32 MFMA sum, ~1e-5 apart; that moves an A element across a bf16 rounding
    midpoint now and then (~0.5 % of them, each moving an output by ~1e-4, a large A times a large weight by up to ~2e-3).  Then:
    99 % of the elements within 1 ulp, every element within 4 ulp with the ulp floor at a quarter of the tensor's RMS (2e-3 at
    RMS 0.47).  One wrong sample -- another level's row, a wrong tap -- moves an output by ~1e-2 and more.

    convs: layers of the (cls, bbox) tower; the deformable layer is the last one, n - 1, its input layer n - 2 after its GroupNorm +
    ReLU (applied in place) or, for a one-layer tower, `pyramid` (the imported features: a tower behind a shared tower is not
    observable then).  norm "none": nn.Sequential step 2, and the stored output is after the epilogue's ReLU, which is folded into the
    expected value.  skip: towers (0 / 1) to leave out.  -> the worst ulp seen."""
    step = 3 if norm == "GN" else 2
    worst = 0.0
    for t, name in ((0, "cls_tower"), (1, "bbox_tower")):
        n = convs[t]
        if n == 0 or t in skip:
            continue
        xs = eng.export_tower(t, n - 2, with_coef=False)[0] if n >= 2 else pyramid
        ys, _ = eng.export_tower(t, n - 1, with_coef=False)
        pre = f"{P}.{name}.{step * (n - 1)}"
        ow = sd[f"{pre}.offset.weight"].bfloat16().double()
        for l in range(len(xs)):
            x = xs[l].cpu()
            om = F.conv2d(x.double(), ow, sd[f"{pre}.offset.bias"].double(), padding=1).float()
            want = DR.deform_conv_bf16(x, om, sd[f"{pre}.conv.weight"], sd[f"{pre}.conv.bias"])
            if step == 2:
                want = F.relu(want)
            want = want.float().bfloat16().float()
            if exact_offsets:
                worst = max(worst, _assert_ulps(ys[l], want, f"{what} {name} level {l}", max_ulp=1.0, max_frac=0.05))
                continue
            ulp1 = _ulps(ys[l], want, 1e-3 * float(want.abs().max()))
            assert float((ulp1 > 1.0).float().mean()) <= 0.01, f"{what} {name} level {l}: {float((ulp1 > 1.0).float().mean()):.4f} > 1 ulp"
            worst = max(worst, _assert_ulps(ys[l], want, f"{what} {name} level {l}", max_ulp=4.0, max_frac=1.0,
                                            floor=0.25 * float(want.pow(2).mean().sqrt())))
    return worst


def test_layer_pinned_bf16_full_pyramid():
    from sylph_amd import synthetic as Wt
    sd = Wt.head_state_dict(seed=3, deformable=True)
    eng = _run_bf16(sd, _feats(2, 17))
    _pin_layer(eng, sd, "bf16 B=2", exact_offsets=False)


def test_borders_read_zeros_not_neighbouring_maps():
    """Constant offsets of up to +-9 px per tap, fractional ones among them (taps leave every map on all four sides, P7 = 7 x 11
    entirely): any read of a row outside the (image, level) map shows up as a non-zero where the restatement has zeros.  Zero
    offset-conv weights make the offsets exact on both sides, so the pin is 1 ulp."""
    from sylph_amd import synthetic as Wt
    sd = Wt.head_state_dict(seed=6, deformable=True)
    shifts = [(-9.0, 0.3), (9.0, -0.6), (0.4, -9.0), (-0.7, 9.0), (-9.0, -9.0), (9.0, 9.0), (3.5, -2.25), (-1.0, 0.0), (0.0, 7.0)]
    for name in ("cls_tower", "bbox_tower"):
        pre = f"{P}.{name}.{K_LAST}"
        sd[f"{pre}.offset.weight"].zero_()
        for j, (dy, dx) in enumerate(shifts):
            sd[f"{pre}.offset.bias"][2 * j] = dy
            sd[f"{pre}.offset.bias"][2 * j + 1] = dx
    eng = _run_bf16(sd, _feats(2, 29))
    _pin_layer(eng, sd, "borders", exact_offsets=True)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_zero_offsets_equal_plain_tower(dtype):
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    sd = Wt.head_state_dict(seed=8, deformable=True)
    plain = Wt.head_state_dict(seed=8)
    for name in ("cls_tower", "bbox_tower"):
        pre = f"{P}.{name}.{K_LAST}"
        sd[f"{pre}.offset.weight"].zero_()
        sd[f"{pre}.offset.bias"].zero_()
        sd[f"{pre}.offset.bias"][18:] = 40.0  # sigmoid(40) == 1.0f
        plain[f"{pre}.weight"] = sd[f"{pre}.conv.weight"]
        plain[f"{pre}.bias"] = sd[f"{pre}.conv.bias"]
    feats = _feats(2, 31)
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    outs = []
    for deformable, w in ((True, sd), (False, plain)):
        eng = Engine(_cfg(deformable), dtype=dtype)
        eng.load_state_dict(w)
        eng.import_pyramid(feats, (H, W))
        eng.head(codes["cls_conv"], codes["cls_bias"])
        outs.append([eng.export_tower(t, 3, with_coef=False)[0] for t in (0, 1)] + [eng.export_head()])
    for t in (0, 1):
        for l in range(5):
            a, b = outs[0][t][l], outs[1][t][l]
            if dtype == "bf16":
                _assert_ulps(a, b, f"tower {t} level {l}", max_ulp=2.0, max_frac=0.05)
            else:
                assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), (t, l)
    tol = 1e-3 if dtype == "f32" else 6e-2
    for fa, fb in zip(outs[0][2], outs[1][2]):
        for a, b in zip(fa, fb):
            assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


SMALL = (384, 640)
SMALL_LEVELS = [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5)]


@pytest.fixture(scope="module")
def f32_case():
    from sylph_amd import synthetic as Wt
    sd = Wt.head_state_dict(seed=12, deformable=True)
    feats = _feats(1, 41, SMALL_LEVELS)
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    want = DR.deform_fcos_head([f.double() for f in feats], sd, codes)
    return sd, feats, codes, want


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_head_f32_matches_restatement_and_decoder(f32_case, dtype):
    from sylph_amd.engine import Engine
    sd, feats, codes, want = f32_case
    eng = Engine(_cfg(), dtype=dtype)
    eng.load_state_dict(sd)
    eng.import_pyramid(feats, SMALL)
    eng.head(codes["cls_conv"], codes["cls_bias"])
    got = eng.export_head()
    worst = 0.0
    for gl, wl in zip(got, want):
        for g, w in zip(gl, wl):
            worst = max(worst, float((g.cpu().double() - w).abs().max()) / max(1.0, float(w.abs().max())))
    print(f"{dtype}: worst head difference {worst:.2e}")
    assert worst <= 1e-3
    mine = eng.decode()
    eng.import_head([w.float() for w in want[0]], [w.float() for w in want[1]], [w.float() for w in want[2]], [w.float() for w in want[3]])
    ref = eng.decode()
    for a, b in zip(mine, ref):
        assert torch.equal(a["cand_index"].cpu(), b["cand_index"].cpu())


def test_batch_position_bit_identical():
    from sylph_amd import synthetic as Wt
    from sylph_amd.engine import Engine
    sd = Wt.head_state_dict(seed=14, deformable=True)
    g = torch.Generator(device="cuda").manual_seed(23)
    one = [torch.randn(1, 256, h, w, generator=g, device="cuda").bfloat16().float() for h, w in LEVELS]
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    ref = None
    for B in (1, 8, 192):
        eng = Engine(_cfg(), dtype="bf16")
        eng.load_state_dict(sd)
        eng.import_pyramid([f.repeat(B, 1, 1, 1) for f in one], (H, W))
        eng.head(codes["cls_conv"], codes["cls_bias"])
        lo, rg, ct, io = eng.export_head()
        outs = [torch.cat([t.flatten(1) for t in ts], 1) for ts in (lo, rg, ct, io)]
        if ref is None:
            ref = [o[:1].clone() for o in outs]
        for o, r in zip(outs, ref):
            bad = (o != r).any(dim=1).nonzero().flatten().tolist()
            assert not bad, f"B={B}: images {bad[:8]} differ from the B=1 result"
        del eng, lo, rg, ct, io, outs
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_models_run_a_deformable_checkpoint(dtype):
    """The episodic model and the base detector (run_type None) on a deformable checkpoint, through the config key alone: the base
    detector gives exactly the detections of the episodic model fed with the checkpoint's cls_logits as class codes."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    sd = Wt.synthetic_state_dict(0, depth=50)
    dfm = Wt.head_state_dict(seed=1, num_classes=int(sd[f"{P}.cls_logits.weight"].shape[0]), deformable=True)
    for name in ("cls_tower", "bbox_tower"):
        sd.pop(f"{P}.{name}.{K_LAST}.weight")
        sd.pop(f"{P}.{name}.{K_LAST}.bias")
        for sfx in (".offset.weight", ".offset.bias", ".conv.weight", ".conv.bias"):
            sd[f"{P}.{name}.{K_LAST}{sfx}"] = dfm[f"{P}.{name}.{K_LAST}{sfx}"]
    r = MetaFCOSRunner()
    ecfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    ecfg.MODEL.FCOS.USE_DEFORMABLE = True
    ecfg.MODEL.FCOS.INFERENCE_TH_TEST = 0.0  # every location is a candidate: POST_NMS_TOPK_TEST detections per image to compare
    epi = r.build_model(ecfg, dtype=dtype)
    epi.load_state_dict(sd)
    epi.eval()
    cfg = r.get_default_cfg()
    cfg.MODEL.FCOS.USE_DEFORMABLE = True
    cfg.MODEL.FCOS.INFERENCE_TH_TEST = 0.0
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = False
    cfg.MODEL.FCOS.CLS_LOGITS_KERNEL_SIZE = 1
    cfg.MODEL.FCOS.NUM_CLASSES = int(sd[f"{P}.cls_logits.weight"].shape[0])
    base = r.build_model(cfg, dtype=dtype)
    base.load_state_dict({k: v for k, v in sd.items() if not k.startswith("code_generator.")})
    base.eval()
    imgs = Wt.synthetic_images(2, 192, 256, seed=22)
    batch = [{"image": im, "height": 192, "width": 256} for im in imgs]
    w, b = sd[f"{P}.cls_logits.weight"], sd[f"{P}.cls_logits.bias"]
    exp = epi(batch, class_code={"cls_conv": w.cuda(), "cls_bias": b.cuda()}, run_type="meta_learn_test_instance")
    got = base(batch)
    assert len(got) == 2
    n = 0
    for x, y in zip(got, exp):
        assert torch.equal(x["instances"].pred_boxes.tensor, y["instances"].pred_boxes.tensor)
        assert torch.equal(x["instances"].scores, y["instances"].scores)
        n += len(x["instances"])
    print(f"{dtype}: {n} detections")
    assert n > 0
