"""ResNeXt backbones on the MI355X: the grouped 3x3 kernel (conv_group.hip) pinned to the bf16 / fp32 restatements of
tests/resnext_ref.py, whole ResNeXt blocks through the backbone's launches, an X-101-32x8d network against the restated oracle in the
parity modes, batch-position and batch-size checks of the 192-image step, and the public entry points on a ResNeXt checkpoint.

Tolerances are those of tests/test_bf16_pinned_gpu.py: one conv with no bf16 intermediate <= 1 ulp of the element (floor 1e-3 of the
tensor's maximum); a block with bf16 intermediates <= 2 ulps at max(|element|, rms)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resnext_ref as XR

pytestmark = pytest.mark.gpu
P = "proposal_generator.fcos_head"


def _cfg(groups=32, wpg=8, depth=101):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = depth, groups, wpg, False
    return cfg


def _engine(dtype, cfg=None):
    from sylph_amd.engine import Engine
    return Engine(cfg if cfg is not None else _cfg(), dtype=dtype)


def _ulps(got, want, floor):
    got, want = got.double().cpu(), want.double().cpu()
    fl = float(want.abs().max()) * 1e-3 if floor == "max" else float(want.pow(2).mean().sqrt())
    mag = torch.clamp(want.abs(), min=fl)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    d = (got - want).abs()
    return float((d > 0).double().mean()), float((d / ulp).max())


def _assert_ulps(got, want, what, max_ulp, max_frac, floor):
    assert got.shape == want.shape, (got.shape, want.shape)
    frac, worst = _ulps(got, want, floor)
    print(f"{what}: {frac * 100:.3f} % differ, worst {worst:.2f} ulp")
    assert worst <= max_ulp and frac <= max_frac, f"{what}: {frac * 100:.3f} % differ, worst {worst:.2f} ulp"


def _layer(g, C, cpg):
    w = torch.randn(C, cpg, 3, 3, generator=g) * (2.0 / (9 * cpg)) ** 0.5
    return w, 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g)


LAYERS = [
    # name, channels per group, C, H, W, stride, batch
    ("X-50-32x4d res2", 4, 128, 200, 336, 1, 1),
    ("X-101-32x8d res2", 8, 256, 200, 336, 1, 1),
    ("X-101-32x8d res3 first (stride 2)", 16, 512, 200, 336, 2, 1),
    ("X-101-32x8d res3 ragged", 16, 512, 93, 157, 1, 2),
    ("X-101-32x8d res4 ragged", 32, 1024, 47, 83, 1, 2),
    ("X-101-32x8d res5 first (stride 2)", 64, 2048, 50, 84, 2, 2),
    ("X-101-32x8d res5", 64, 2048, 25, 42, 1, 3),
    ("X-101-64x4d res2 ragged stride 2", 4, 256, 37, 61, 2, 3),
]


@pytest.mark.parametrize("case", LAYERS, ids=[c[0].replace(" ", "_") for c in LAYERS])
def test_grouped_layer_pinned_bf16(case):
    name, cpg, C, h, w, stride, B = case
    g = torch.Generator().manual_seed(C + cpg + stride)
    x = XR.OB16.r(F.relu(torch.randn(B, C, h, w, generator=g)))
    wt, sc, sh = _layer(g, C, cpg)
    y = _engine("bf16").group_conv(x, wt, sc, sh, C // cpg, stride=stride).cpu()
    want = XR.conv_epilogue_grouped(x, wt, sc, sh, C // cpg, stride=stride)
    _assert_ulps(y, want, name, max_ulp=1.0, max_frac=0.01, floor="max")


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("case", [LAYERS[0], LAYERS[2], LAYERS[4], LAYERS[6], LAYERS[7]], ids=lambda c: c[0].replace(" ", "_"))
def test_grouped_layer_f32(case, dtype):
    name, cpg, C, h, w, stride, B = case
    g = torch.Generator().manual_seed(C + cpg + stride)
    x = F.relu(torch.randn(B, C, h, w, generator=g))
    wt, sc, sh = _layer(g, C, cpg)
    y = _engine(dtype).group_conv(x, wt, sc, sh, C // cpg, stride=stride, relu=False).cpu().double()
    want = F.conv2d(x.double(), wt.double(), None, stride=stride, padding=1, groups=C // cpg) * sc.double().view(1, -1, 1, 1) + \
        sh.double().view(1, -1, 1, 1)
    err = float((y - want).abs().max()) / float(want.abs().max())
    print(f"{name} {dtype}: relative max error {err:.2e}")
    assert err <= 1e-5


BLOCKS = [
    # name, Cin, mid, cout, H, W, stride, shortcut, groups, batch
    ("X-101-32x8d res2 first (projection)", 64, 256, 256, 200, 336, 1, True, 32, 1),
    ("X-101-32x8d res2 identity", 256, 256, 256, 200, 336, 1, False, 32, 1),
    ("X-101-32x8d res3 first (stride 2 on the grouped conv)", 256, 512, 512, 200, 336, 2, True, 32, 1),
    ("X-50-32x4d res3 identity (mid 256)", 512, 256, 512, 100, 168, 1, False, 32, 2),
    ("X-101-32x8d res4 first", 512, 1024, 1024, 100, 168, 2, True, 32, 1),
    ("X-101-32x8d res5 first", 1024, 2048, 2048, 50, 84, 2, True, 32, 2),
    ("X-101-32x8d res5 identity ragged", 2048, 2048, 2048, 23, 37, 1, False, 32, 2),
    # batches whose 1x1 launches take conv_pw / conv_spw (>= 256 / 512 M tiles) at the new widths
    ("X-101-32x8d res2 identity B4 (conv_pw conv1, conv_spw conv3)", 256, 256, 256, 200, 336, 1, False, 32, 4),
    ("X-101-32x8d res3 identity B8 (conv_pw conv1, conv_spw conv3)", 512, 512, 512, 100, 168, 1, False, 32, 8),
    ("X-101-32x8d res3 first B4 (conv3 + projection on conv_pw)", 256, 512, 512, 200, 336, 2, True, 32, 4),
]


@pytest.mark.parametrize("case", BLOCKS, ids=[c[0].split(" (")[0].replace(" ", "_") for c in BLOCKS])
def test_grouped_block_pinned_bf16(case):
    name, cin, mid, cout, h, w, stride, shortcut, G, B = case
    g = torch.Generator().manual_seed(cin + mid + stride)
    x = XR.OB16.r(F.relu(torch.randn(B, cin, h, w, generator=g)))
    ws = [torch.randn(mid, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5,
          torch.randn(mid, mid // G, 3, 3, generator=g) * (2.0 / (9 * mid // G)) ** 0.5,
          torch.randn(cout, mid, 1, 1, generator=g) * (2.0 / mid) ** 0.5]
    if shortcut:
        ws.append(torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5)
    scales = [0.5 + torch.rand(t.shape[0], generator=g) for t in ws]
    shifts = [0.2 * torch.randn(t.shape[0], generator=g) for t in ws]
    y = _engine("bf16").bottleneck_grouped(x, ws, scales, shifts, stride, groups=G).cpu()
    want = XR.bottleneck_bf16(x, ws, scales, shifts, stride, G, stride_in_1x1=False)
    _assert_ulps(y, want, name, max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.fixture(scope="module")
def x101_sd():
    from sylph_amd import synthetic as Wt
    sd = Wt.backbone_state_dict(0, depth=101, num_groups=32, width_per_group=8)
    sd.update(Wt.head_state_dict(1, num_classes=60))
    return sd


@pytest.fixture(scope="module")
def x101_full(x101_sd):
    """800x1333 + a ragged 750x1200 image: the restated X-101-32x8d backbone (fp32) and the oracle head on it."""
    from oracle import backbone as OB, head as OH
    from sylph_amd import synthetic as Wt
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except AttributeError:
        pass
    q = Wt.synthetic_images(2, 800, 1333, seed=3)
    q[1] = q[1][:, :750, :1200].contiguous()
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    x, sizes = OB.preprocess(q)
    with torch.no_grad():
        pyr = XR.resnext_backbone_fpn(x, x101_sd, 101, 32)
        head = OH.fcos_head(pyr, x101_sd, codes)
    return q, codes, sizes, pyr, head


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_x101_full_size_matches_restatement(x101_sd, x101_full, dtype):
    from oracle import decode as OD
    q, codes, sizes, pyr, ref_head = x101_full
    eng = _engine(dtype)
    eng.load_state_dict(x101_sd)
    assert eng.preprocess(q) == (800, 1344)
    eng.backbone()
    for l, (a, b) in enumerate(zip(eng.export_pyramid(), pyr)):  # 101 layers of fp32 sums: 1e-3 of the level's scale
        err = float((a.cpu() - b).abs().max()) / max(1.0, float(b.abs().max()))
        assert err <= 1e-3, f"{dtype} p{l + 3}: max err {err} of the level's scale"
    eng.head(codes["cls_conv"], codes["cls_bias"])
    hip_head = [[t.cpu() for t in ts] for ts in eng.export_head()]
    for name, hs, rs in zip(("logits", "reg", "ctrness", "iou"), hip_head, ref_head):
        for l in range(5):
            err = float((hs[l] - rs[l]).abs().max())
            assert err <= 1e-3, f"{dtype} {name} level {l}: max err {err}"
    got = eng.decode()
    want = OD.predict_proposals(*hip_head)
    for i in range(2):
        wh = OD.detector_postprocess(want[i], sizes[i], sizes[i][0], sizes[i][1])
        assert got[i]["scores"].numel() == wh["scores"].numel() > 0
        np.testing.assert_array_equal(got[i]["pred_classes"].cpu().numpy(), wh["pred_classes"].numpy())
        np.testing.assert_array_equal(got[i]["fpn_levels"].cpu().numpy(), wh["fpn_levels"].numpy())
        np.testing.assert_allclose(got[i]["scores"].cpu().numpy(), wh["scores"].numpy(), atol=1e-5)
        np.testing.assert_allclose(got[i]["pred_boxes"].cpu().numpy(), wh["pred_boxes"].numpy(), atol=1e-3)


def _step(sd, imgs, codes, keep):
    """One bf16 query step; returns the pyramid and the head outputs of images [0, keep) (device), whether every later group of `keep`
    images equals the first bit for bit (pyramid, head outputs, detections), and the detections of images [0, keep)."""
    eng = _engine("bf16")
    eng.load_state_dict(sd)
    eng.preprocess(imgs)
    eng.backbone()
    pyr = eng.export_pyramid()
    same = all(torch.equal(p[:keep], p[k:k + keep]) for p in pyr for k in range(keep, len(imgs), keep))
    pyr = [p[:keep].clone() for p in pyr]
    eng.head(codes["cls_conv"], codes["cls_bias"])
    outs = [torch.cat([t.flatten(1) for t in ts], 1) for ts in eng.export_head()]
    same = same and all(torch.equal(o[:keep], o[k:k + keep]) for o in outs for k in range(keep, len(imgs), keep))
    outs = [o[:keep].clone() for o in outs]
    dets = [{k: v.cpu() for k, v in d.items() if torch.is_tensor(v)} for d in eng.decode()]
    same = same and all(torch.equal(dets[i][k], dets[i % keep][k]) for i in range(keep, len(imgs)) for k in dets[i])
    eng.close()
    del eng
    torch.cuda.empty_cache()
    return pyr, outs, same, dets[:keep]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_batch_192_x101_positions_and_batch_sizes(x101_sd, x101_full):
    """One bf16 step of 192 full-size X-101-32x8d images: four images (the first is the 800x1333 image of x101_full) repeated 48 times.
      * every copy gives the same bits wherever it sits (pyramid, head outputs, detections) -- the oversized blocks run as image chunks;
      * 8-image and 1-image steps: launches of few tiles take other routes (the res4 / res5 1x1 layers of one image run on conv_igemm
        instead of conv_pw / conv_spw, the FPN P6 / P7 convs of small batches are split along K), whose fp32 sums over K run in
        another order; the bf16 roundings that differ spread through the following blocks.  Held to the bar of
        test_headline_batch_gpu.py (pyramid within 4e-2 of each level's scale) and to 2e-2 relative L2 on the logits (measured for
        image 0, B = 1 against B = 64: R-101 7.6e-3, X-101-32x8d 8.5e-3);
      * against the fp32 restatement of the network (x101_full), image 0's bf16 pyramid is within 5e-2 relative L2 per level: bf16
        storage through 101 blocks, where a wrong route or operand is O(1)."""
    from sylph_amd import synthetic as Wt
    q, codes, sizes, pyr_ref, _ = x101_full
    four = [q[0]] + Wt.synthetic_images(3, 800, 1333, seed=11)
    p192, o192, same, d192 = _step(x101_sd, [four[i % 4] for i in range(192)], codes, 4)
    assert same, "a copy in the 192-image step differs from images 0-3"
    assert all(d["scores"].numel() > 0 for d in d192)
    p8, o8, same8, _ = _step(x101_sd, [four[i % 4] for i in range(8)], codes, 4)
    assert same8
    p1, o1, _, _ = _step(x101_sd, four[:1], codes, 1)
    for B, ps, os_ in ((8, p8, o8), (1, p1, o1)):
        n = ps[0].shape[0]
        for l, (a, b) in enumerate(zip(ps, p192)):
            err = float((a - b[:n]).abs().max()) / float(b[:n].abs().max())
            print(f"p{l + 3}: B = {B} vs B = 192 max err {err:.2e} of the level's scale (bit-identical: {torch.equal(a, b[:n])})")
            assert err <= 4e-2
        rel = _rel(os_[0], o192[0][:n])
        print(f"logits: B = {B} vs B = 192 relative L2 {rel:.2e}")
        assert rel <= 2e-2
    for l, (a, b) in enumerate(zip(p192, pyr_ref)):
        rel = _rel(a[0].cpu(), b[0])
        print(f"p{l + 3}: bf16 B = 192 vs fp32 restatement relative L2 {rel:.2e}")
        assert rel <= 5e-2


def test_runner_episode_and_predictor_on_resnext(x101_sd, tmp_path):
    """MetaFCOSRunner (support -> codes -> query) and SylphPredictor on an X-50-32x4d checkpoint give the engine's detections."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.data import SyntheticSupportSetLoader
    from sylph_amd.engine import Engine
    from sylph_amd.evaluation import inference_normalization, inference_on_support_set_dataset
    from sylph_amd.predictor import SylphPredictor, resize_image, resize_shortest_edge_shape
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    sd = Wt.synthetic_state_dict(0, depth=50)
    sd.update(Wt.backbone_state_dict(0, depth=50, num_groups=32, width_per_group=4))
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    rr = cfg.MODEL.RESNETS
    rr.DEPTH, rr.NUM_GROUPS, rr.WIDTH_PER_GROUP, rr.STRIDE_IN_1X1 = 50, 32, 4, False
    model = r.build_model(cfg, dtype="f32")
    model.load_state_dict(sd)
    model.eval()
    sub = inference_on_support_set_dataset(model, SyntheticSupportSetLoader(2, 1, 128, 160, seed=5), output_dir=None)
    sub = inference_normalization(model, sub)
    code_dir = str(tmp_path / "codes" / "synthetic_all" / "0")
    os.makedirs(code_dir)
    for c in sub:
        c["class_code"] = {k: v.cpu() for k, v in c["class_code"].items()}
        c["class_code"]["cls_conv"] = c["class_code"]["cls_conv"] * 3.0
        torch.save(c, os.path.join(code_dir, f"{c['class_name']}.pth"))
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": sd}, ckpt)
    yaml = str(tmp_path / "x50.yaml")
    with open(yaml, "w") as f:
        f.write(cfg.dump())
    pred = SylphPredictor(yaml, ckpt, str(tmp_path / "codes"), test_dataset_names={"all": "synthetic_all"}, dtype="f32")
    pred.min_size, pred.max_size = 96, 160
    img = np.random.RandomState(0).randint(0, 256, size=(90, 130, 3), dtype=np.uint8)
    out = pred._call_few_shot(img, pred.class_codes["all"])["instances"]
    nh, nw = resize_shortest_edge_shape(90, 130, 96, 160)
    x = torch.as_tensor(resize_image(img, nh, nw).astype("float32").transpose(2, 0, 1))
    codes = {k: v.cuda() for k, v in pred.class_codes["all"].items()}
    eng = Engine(cfg, dtype="f32")
    eng.load_state_dict(sd)
    eng.preprocess([x])
    eng.backbone()
    eng.head(codes["cls_conv"], codes["cls_bias"])
    want = eng.decode()[0]
    assert len(out) == want["scores"].numel() > 0
    np.testing.assert_allclose(np.sort(out.scores.cpu().numpy()), np.sort(want["scores"].cpu().numpy()), atol=1e-5)
    # the runner's query path on the same image and codes
    got = model([{"image": x, "height": nh, "width": nw}], class_code={k: v for k, v in codes.items()},
                run_type="meta_learn_test_instance")[0]["instances"]
    assert len(got) == want["scores"].numel()
    np.testing.assert_allclose(np.sort(got.scores.cpu().numpy()), np.sort(want["scores"].cpu().numpy()), atol=1e-5)


def test_caffe2_resnext_checkpoint_loads_and_wrong_conv2_shape_names_the_key(tmp_path):
    import pickle
    from sylph_amd import synthetic as Wt
    from sylph_amd.checkpoint import load_checkpoint_file
    from tests.test_host_cpu import _to_caffe2
    sd = Wt.backbone_state_dict(0, depth=50, num_groups=32, width_per_group=4)
    path = str(tmp_path / "X-50-32x4d.pkl")
    with open(path, "wb") as f:
        pickle.dump(_to_caffe2(sd), f)
    loaded = load_checkpoint_file(path)
    assert tuple(loaded["backbone.bottom_up.res3.2.conv2.weight"].shape) == (256, 8, 3, 3)
    assert torch.equal(loaded["backbone.bottom_up.res3.2.conv2.weight"], sd["backbone.bottom_up.res3.2.conv2.weight"])
    loaded.update({k: v for k, v in sd.items() if not k.startswith("backbone.bottom_up.")})
    imgs = Wt.synthetic_images(1, 64, 96, seed=2)
    eng = _engine("f32", _cfg(32, 4, 50))
    eng.load_state_dict(loaded)
    eng.preprocess(imgs)
    eng.backbone()
    assert all(torch.isfinite(p).all() for p in eng.export_pyramid())
    # an R-50 checkpoint under the ResNeXt config, and the ResNeXt one under the plain config: the conv2 key is named
    r50 = Wt.backbone_state_dict(0, depth=50)
    with pytest.raises(RuntimeError, match=r"res2\.0\.conv2\.weight"):
        _engine("bf16", _cfg(32, 4, 50)).load_state_dict(r50)
    with pytest.raises(RuntimeError, match=r"res2\.0\.conv2\.weight"):
        _engine("bf16", _cfg(1, 64, 50)).load_state_dict(sd)
