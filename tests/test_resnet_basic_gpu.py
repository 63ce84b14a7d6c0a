"""ResNet-18 / ResNet-34 backbones on the MI355X: the 64-channel 3x3 kernel (conv_rw64.hip) pinned to the bf16 / float64 restatements,
whole BasicBlocks through the backbone's launches (with the routes they take asserted), whole R-18 / R-34 networks against the
restated oracle (tests/basic_ref.py) in the parity modes, batch-position and batch-size checks of the 192-image step, and the public
entry points on an R-18 checkpoint.

Tolerances are those of tests/test_bf16_pinned_gpu.py: one conv with no bf16 intermediate <= 1 ulp of the element (floor 1e-3 of the
tensor's maximum); a block with bf16 intermediates <= 2 ulps at max(|element|, rms)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bf16 as OB16
from tests import basic_ref as BR

pytestmark = pytest.mark.gpu
KERNEL = "conv_rw64_kernel"


def _cfg(depth=18):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.RES2_OUT_CHANNELS = depth, 64
    return cfg


def _engine(dtype, cfg=None, profile=False):
    from sylph_amd.engine import Engine
    eng = Engine(cfg if cfg is not None else _cfg(), dtype=dtype)
    if profile:
        eng.profile_enable(True)
    return eng


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


def _layer(g, cout, cin, k=3):
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    return w, 0.5 + torch.rand(cout, generator=g), 0.2 * torch.randn(cout, generator=g)


LAYERS = [
    # name, H, W, batch
    ("res2 200x336 B1", 200, 336, 1),
    ("res2 200x336 B4", 200, 336, 4),
    ("ragged 93x157 B2", 93, 157, 2),
    ("ragged 37x61 B3", 37, 61, 3),
]


def _layer_operands(case, residual, bf16=True):
    name, h, w, B = case
    g = torch.Generator().manual_seed(h * 7 + w + B + int(residual))
    x = F.relu(torch.randn(B, 64, h, w, generator=g))
    res = F.relu(torch.randn(B, 64, h, w, generator=g)) if residual else None
    if bf16:
        x, res = OB16.r(x), (OB16.r(res) if residual else None)
    return (x, res) + _layer(g, 64, 64)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", LAYERS, ids=[c[0].replace(" ", "_") for c in LAYERS])
def test_conv64_kernel_pinned_bf16(case, residual, monkeypatch):
    monkeypatch.setenv("SYLPH_CONV_RW64", "2")  # forced: the small ragged cases sit below the auto threshold
    x, res, wt, sc, sh = _layer_operands(case, residual)
    eng = _engine("bf16", profile=True)
    y = eng.conv3x3_c64(x, wt, sc, sh, relu=True, residual=res).cpu()
    kernels = eng.profile_read()["kernels"]
    assert list(kernels) == [KERNEL] and kernels[KERNEL]["launches"] == 1, kernels
    _, want = OB16.conv_epilogue(x, wt, sc, sh, padding=1, relu=True, res_bf=res)
    _assert_ulps(y, want, f"conv_rw64 {case[0]} residual={residual}", max_ulp=1.0, max_frac=0.01, floor="max")


def test_conv64_without_relu(monkeypatch):
    """the entry's relu switch: negative outputs survive, and the residual is added before the rounding"""
    monkeypatch.setenv("SYLPH_CONV_RW64", "2")
    x, res, wt, sc, sh = _layer_operands(LAYERS[2], True)
    y = _engine("bf16").conv3x3_c64(x, wt, sc, sh - 1.0, relu=False, residual=res).cpu()
    _, want = OB16.conv_epilogue(x, wt, sc, sh - 1.0, padding=1, relu=False, res_bf=res)
    assert float(want.min()) < 0
    _assert_ulps(y, want, "conv_rw64 without ReLU", max_ulp=1.0, max_frac=0.01, floor="max")


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_conv64_switch_off_takes_the_generic_route(residual, monkeypatch):
    monkeypatch.setenv("SYLPH_CONV_RW64", "0")
    x, res, wt, sc, sh = _layer_operands(LAYERS[0], residual)
    eng = _engine("bf16", profile=True)
    y = eng.conv3x3_c64(x, wt, sc, sh, relu=True, residual=res).cpu()
    kernels, routes = eng.profile_read()["kernels"], eng.conv_routes()
    assert KERNEL not in kernels and len(routes) == 1 and routes[0].split()[0] in ("igemm", "igemm_halo", "igemm_splitk"), (kernels, routes)
    _, want = OB16.conv_epilogue(x, wt, sc, sh, padding=1, relu=True, res_bf=res)
    _assert_ulps(y, want, f"generic route residual={residual}", max_ulp=1.0, max_frac=0.01, floor="max")


def test_conv64_auto_threshold_sides(monkeypatch):
    """auto (the default): an eight-image res2 launch (2 176 patches) runs on the kernel, a four-image one (1 088) and a 37 x 61 map
    do not"""
    monkeypatch.delenv("SYLPH_CONV_RW64", raising=False)
    eng = _engine("bf16", profile=True)
    for case, on in ((("res2 200x336 B8", 200, 336, 8), True), (LAYERS[1], False), (LAYERS[3], False)):
        x, res, wt, sc, sh = _layer_operands(case, False)
        eng.conv3x3_c64(x, wt, sc, sh)
        assert (KERNEL in eng.profile_read()["kernels"]) == on, case[0]


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("case", [LAYERS[0], LAYERS[3]], ids=lambda c: c[0].replace(" ", "_"))
def test_conv64_f32(case, dtype):
    x, res, wt, sc, sh = _layer_operands(case, True, bf16=False)
    eng = _engine(dtype, profile=True)
    y = eng.conv3x3_c64(x, wt, sc, sh, relu=False, residual=res).cpu().double()
    assert KERNEL not in eng.profile_read()["kernels"]
    want = F.conv2d(x.double(), wt.double(), None, padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) + res.double()
    err = float((y - want).abs().max()) / float(want.abs().max())
    print(f"{case[0]} {dtype}: relative max error {err:.2e}")
    assert err <= 1e-5


BLOCKS = [
    # name, Cin, cout, H, W, stride, batch, kernel that must run (or None), route that must appear (or None)
    ("res2 identity B8", 64, 64, 200, 336, 1, 8, KERNEL, None),
    ("res2 identity B1 (below the kernel's threshold)", 64, 64, 200, 336, 1, 1, None, "igemm"),
    ("res3 first (stride 2, projection)", 64, 128, 200, 336, 2, 1, None, None),
    ("res3 identity (conv_rw3 conv1)", 128, 128, 100, 168, 1, 2, "conv_rw3_kernel", None),
    ("res4 first B6", 128, 256, 100, 168, 2, 6, None, None),
    ("res4 identity B6 (conv_hpipe conv1)", 256, 256, 50, 84, 1, 6, None, "hpipe"),
    ("res5 identity ragged", 512, 512, 23, 37, 1, 2, None, None),
]


@pytest.mark.parametrize("case", BLOCKS, ids=[c[0].split(" (")[0].replace(" ", "_") for c in BLOCKS])
def test_basic_block_pinned_bf16(case, monkeypatch):
    monkeypatch.delenv("SYLPH_CONV_RW64", raising=False)
    name, cin, cout, h, w, stride, B, kernel, route = case
    shortcut = cin != cout
    g = torch.Generator().manual_seed(cin + cout + stride)
    x = OB16.r(F.relu(torch.randn(B, cin, h, w, generator=g)))
    layers = [_layer(g, cout, cin), _layer(g, cout, cout)] + ([_layer(g, cout, cin, 1)] if shortcut else [])
    ws, scales, shifts = [[l[i] for l in layers] + ([] if shortcut else [None]) for i in range(3)]
    eng = _engine("bf16", profile=True)
    y = eng.basic_block(x, ws, scales, shifts, stride).cpu()
    kernels, routes = eng.profile_read()["kernels"], eng.conv_routes()
    print(f"{name}: kernels {sorted(kernels)}, routes {routes}")
    if kernel:
        assert kernel in kernels, (kernels, routes)
    if kernel == KERNEL:
        assert kernels[KERNEL]["launches"] == 2 and not routes  # conv1 and conv2, nothing on the generic routes
    if route:
        assert routes and routes[0].startswith(route), routes
    want = BR.basic_block_bf16(x, ws, scales, shifts, stride)
    _assert_ulps(y, want, name, max_ulp=2.0, max_frac=0.03, floor="rms")


_FULL = {}


def _full(depth):
    """800x1333 + a ragged 750x1200 image: the restated R-18 / R-34 backbone (fp32) and the oracle head on it (computed once per depth)."""
    if depth in _FULL:
        return _FULL[depth]
    from oracle import backbone as OB, head as OH
    from sylph_amd import synthetic as Wt
    try:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    except AttributeError:
        pass
    sd = Wt.backbone_state_dict(0, depth=depth)
    sd.update(Wt.head_state_dict(1, num_classes=60))
    q = Wt.synthetic_images(2, 800, 1333, seed=3)
    q[1] = q[1][:, :750, :1200].contiguous()
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    x, sizes = OB.preprocess(q)
    with torch.no_grad():
        pyr = BR.basic_backbone_fpn(x, sd, depth)
        head = OH.fcos_head(pyr, sd, codes)
    _FULL[depth] = (depth, sd, q, codes, sizes, pyr, head)
    return _FULL[depth]


@pytest.fixture(scope="module", params=[18, 34], ids=["R18", "R34"])
def basic_full(request):
    return _full(request.param)


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_full_size_matches_restatement(basic_full, dtype):
    from oracle import decode as OD
    depth, sd, q, codes, sizes, pyr, ref_head = basic_full
    eng = _engine(dtype, _cfg(depth))
    eng.load_state_dict(sd)
    assert eng.preprocess(q) == (800, 1344)
    eng.backbone()
    assert tuple(eng.export_stage(2).shape) == (2, 64, 200, 336) and tuple(eng.export_stage(5).shape) == (2, 512, 25, 42)
    for l, (a, b) in enumerate(zip(eng.export_pyramid(), pyr)):
        err = float((a.cpu() - b).abs().max()) / max(1.0, float(b.abs().max()))
        assert err <= 1e-3, f"R-{depth} {dtype} p{l + 3}: max err {err} of the level's scale"
    eng.head(codes["cls_conv"], codes["cls_bias"])
    hip_head = [[t.cpu() for t in ts] for ts in eng.export_head()]
    for name, hs, rs in zip(("logits", "reg", "ctrness", "iou"), hip_head, ref_head):
        for l in range(5):
            err = float((hs[l] - rs[l]).abs().max())
            assert err <= 1e-3, f"R-{depth} {dtype} {name} level {l}: max err {err}"
    got = eng.decode()
    want = OD.predict_proposals(*hip_head)
    for i in range(2):
        wh = OD.detector_postprocess(want[i], sizes[i], sizes[i][0], sizes[i][1])
        assert got[i]["scores"].numel() == wh["scores"].numel() > 0
        np.testing.assert_array_equal(got[i]["pred_classes"].cpu().numpy(), wh["pred_classes"].numpy())
        np.testing.assert_array_equal(got[i]["fpn_levels"].cpu().numpy(), wh["fpn_levels"].numpy())
        np.testing.assert_allclose(got[i]["scores"].cpu().numpy(), wh["scores"].numpy(), atol=1e-5)
        np.testing.assert_allclose(got[i]["pred_boxes"].cpu().numpy(), wh["pred_boxes"].numpy(), atol=1e-3)


def test_export_stage_bf16_tracks_bf16_restatement(basic_full, monkeypatch):
    """res2 of a bf16 R-18 / R-34 pass (stem + the conv_rw64 blocks) against the bf16 form of the restatement.  Both round at the same
    k = 1 + 2 * blocks stores (stem, two convs per block); they differ only where a value sits on a rounding boundary, and each store
    adds at most 2^-9 relative error (oracle/bf16.py), so k * 2^-9 relative L2 bounds the stage; a wrong operand is O(1)."""
    from oracle import bf16 as OB16m
    depth, sd, q, codes, sizes, pyr, _ = basic_full
    monkeypatch.setenv("SYLPH_CONV_RW64", "2")  # (a one-image step sits below the auto threshold)
    eng = _engine("bf16", _cfg(depth), profile=True)
    eng.load_state_dict(sd)
    eng.preprocess(q[:1])
    eng.backbone()
    kernels = eng.profile_read()["kernels"]
    assert kernels[KERNEL]["launches"] == 2 * BR.STAGE_BLOCKS[depth][0], kernels
    x, _ = OB16m.preprocess(q[:1])
    with torch.no_grad():
        want = BR.resnet_bf16(x, sd, depth)["res2"]
    got = eng.export_stage(2).cpu()
    rel = float((got.double() - want.double()).norm() / want.double().norm())
    print(f"R-{depth} res2 bf16 vs bf16 restatement: relative L2 {rel:.2e}")
    assert rel <= (1 + 2 * BR.STAGE_BLOCKS[depth][0]) * 2.0 ** -9


def _step(sd, imgs, codes, keep):
    """One bf16 R-18 query step; returns the pyramid and the head outputs of images [0, keep) (device), whether every later group of
    `keep` images equals the first bit for bit (pyramid, head outputs, detections), and the detections of images [0, keep)."""
    eng = _engine("bf16", _cfg(18))
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


def test_batch_192_r18_positions_and_batch_sizes():
    """One bf16 step of 192 full-size R-18 images: four images (the first is the 800x1333 image of basic_full) repeated 48 times.
      * every copy gives the same bits wherever it sits (pyramid, head outputs, detections);
      * 8-image and 1-image steps take other routes for the small launches (fp32 sums over K in another order): pyramid within 4e-2
        of each level's scale and 2e-2 relative L2 on the logits of the B = 192 result (the bars of the X-101 test);
      * against the fp32 restatement, image 0's bf16 pyramid is within 5e-2 relative L2 per level."""
    from sylph_amd import synthetic as Wt
    depth, sd, q, codes, sizes, pyr_ref, _ = _full(18)
    four = [q[0]] + Wt.synthetic_images(3, 800, 1333, seed=11)
    p192, o192, same, d192 = _step(sd, [four[i % 4] for i in range(192)], codes, 4)
    assert same, "a copy in the 192-image step differs from images 0-3"
    assert all(d["scores"].numel() > 0 for d in d192)
    p8, o8, same8, _ = _step(sd, [four[i % 4] for i in range(8)], codes, 4)
    assert same8
    p1, o1, _, _ = _step(sd, four[:1], codes, 1)
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


def test_runner_episode_and_predictor_on_r18(tmp_path):
    """MetaFCOSRunner (support -> codes -> query) and SylphPredictor on an R-18 checkpoint give the engine's detections."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.data import SyntheticSupportSetLoader
    from sylph_amd.engine import Engine
    from sylph_amd.evaluation import inference_normalization, inference_on_support_set_dataset
    from sylph_amd.predictor import SylphPredictor, resize_image, resize_shortest_edge_shape
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    sd = Wt.synthetic_state_dict(0, depth=18)
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    rr = cfg.MODEL.RESNETS
    rr.DEPTH, rr.RES2_OUT_CHANNELS = 18, 64
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
    yaml = str(tmp_path / "r18.yaml")
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
    got = model([{"image": x, "height": nh, "width": nw}], class_code={k: v for k, v in codes.items()},
                run_type="meta_learn_test_instance")[0]["instances"]
    assert len(got) == want["scores"].numel()
    np.testing.assert_allclose(np.sort(got.scores.cpu().numpy()), np.sort(want["scores"].cpu().numpy()), atol=1e-5)


def test_wrong_block_type_names_the_key():
    """a bottleneck checkpoint under DEPTH 18, and an R-18 checkpoint under DEPTH 50: the first mismatching key and the shape it needs"""
    from sylph_amd import synthetic as Wt
    from sylph_amd.config import get_default_cfg
    r50, r18 = Wt.backbone_state_dict(0, depth=50), Wt.backbone_state_dict(0, depth=18)
    with pytest.raises(RuntimeError, match=r"res2\.0\.conv1\.weight.*\(64, 64, 3, 3\)"):
        _engine("bf16", _cfg(18)).load_state_dict(r50)
    with pytest.raises(RuntimeError, match=r"res2\.0\.conv1\.weight.*\(64, 64, 1, 1\)"):
        _engine("bf16", get_default_cfg()).load_state_dict(r18)
    # R-18 weights under DEPTH 34: res2.2 does not exist
    with pytest.raises(RuntimeError, match=r"res2\.2\.conv1\.weight"):
        _engine("f32", _cfg(34)).load_state_dict(r18)
