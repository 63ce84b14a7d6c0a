"""MobileNetV2 backbones on the MI355X: the depthwise 3x3 kernel (conv_dw.hip) pinned to float64, every distinct InvertedResidual block
shape of the network through the backbone's launches against the bf16 restatement (tests/mobilenet_ref.py), the zero padding of the
HIDDEN tensor, batch position, whole networks in the parity modes against the fp32 restatement, the bf16 network block by block, and the
public entry points on a MobileNetV2 checkpoint.

Tolerances are those of tests/test_resnet_basic_gpu.py: one conv with no bf16 intermediate <= 1 ulp of the element (floor 1e-3 of the
tensor's maximum); a block with bf16 intermediates <= 2 ulps at max(|element|, rms), at most 3 % of the elements differing."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bf16 as OB16
from tests import mobilenet_ref as MR
from tests.test_resnet_basic_gpu import _assert_ulps, _ulps

pytestmark = pytest.mark.gpu
DW = "dwconv3x3_kernel"
STEM = "mbv2_stem_kernel"


def _cfg():
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = ["", "", 1]
    cg.BIAS_LAYER = ["", "", 1]
    cfg.MODEL.MOBILENET = True
    return cfg


def _engine(dtype, profile=False):
    from sylph_amd.engine import Engine
    eng = Engine(_cfg(), dtype=dtype)
    if profile:
        eng.profile_enable(True)
    return eng


@pytest.fixture(scope="module")
def bf16_engine():
    eng = _engine("bf16", profile=True)
    yield eng
    eng.close()


# ---- the depthwise kernel alone ------------------------------------------------------------------------------------------------------
DW_MAPS = [(1, 1, 1), (2, 3, 1), (37, 61, 3), (64, 50, 1)]  # H, W, batch


def _dw_operands(C, h, w, B, stride):
    g = torch.Generator().manual_seed(C * 1000 + h * 7 + w + stride)
    x = 2.0 + 3.0 * torch.randn(B, C, h, w, generator=g)  # the stored expand output: both clamps of the ReLU6 on load have work
    wt = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    return x, wt, 0.5 + torch.rand(C, generator=g), 1.0 + 0.5 * torch.randn(C, generator=g)


def _dw_f64(x, wt, sc, sh, stride):
    acc = F.conv2d(x.double().clamp(0, 6), wt.double(), None, stride=stride, padding=1, groups=x.shape[1])
    return (acc * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).clamp(0, 6)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [32, 160])
@pytest.mark.parametrize("hwb", DW_MAPS, ids=lambda m: f"{m[0]}x{m[1]}_B{m[2]}")
def test_dwconv3x3_pinned_bf16(bf16_engine, hwb, C, stride):
    h, w, B = hwb
    x, wt, sc, sh = _dw_operands(C, h, w, B, stride)
    x, wt = OB16.r(x), OB16.r(wt)
    eng = bf16_engine
    eng.profile_read()
    y = eng.dwconv3x3(x, wt, sc, sh, stride).cpu()
    kernels = eng.profile_read()["kernels"]
    assert list(kernels) == [DW] and kernels[DW]["launches"] == 1, kernels
    want = _dw_f64(x, wt, sc, sh, stride)
    assert y.shape == want.shape == (B, C, (h - 1) // 2 + 1 if stride == 2 else h, (w - 1) // 2 + 1 if stride == 2 else w)
    if h * w * B > 100:
        assert 0.01 < float((want == 6).double().mean()) < 0.6 and 0.1 < float((want == 0).double().mean()) < 0.9
    _assert_ulps(y, OB16.r(want.float()), f"dwconv3x3 C{C} {h}x{w} B{B} s{stride}", max_ulp=1.0, max_frac=0.01, floor="max")


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv3x3_f32(dtype, stride):
    x, wt, sc, sh = _dw_operands(160, 37, 61, 3, stride)
    eng = _engine(dtype)
    y = eng.dwconv3x3(x, wt, sc, sh, stride).cpu().double()
    want = _dw_f64(x, wt, sc, sh, stride)
    err = float((y - want).abs().max()) / float(want.abs().max())
    print(f"dwconv3x3 {dtype} stride {stride}: relative max error {err:.2e}")
    assert err <= 1e-5


# ---- whole blocks ----------------------------------------------------------------------------------------------------------------------
BLOCK_MAPS = [(37, 61, 3), (22, 14, 2), (45, 70, 1), (2, 3, 1)]


def _block_operands(shape, h, w, B, shift0=(1.0, 0.5)):
    cin, t, cout, stride = shape
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + stride + h)
    hid = cin * t
    x = torch.randn(B, cin, h, w, generator=g)
    if t == 1:
        x = (1.0 + 3.0 * x).clamp(0, 6)  # features.1 reads the ReLU6 output of features.0
    ws = [None if t == 1 else torch.randn(hid, cin, 1, 1, generator=g) * (3.0 / cin ** 0.5),
          torch.randn(hid, 1, 3, 3, generator=g) * 0.4, torch.randn(cout, hid, 1, 1, generator=g) * (0.4 / hid ** 0.5)]
    chans = [hid, hid, cout]
    scales = [None if ws[i] is None else 0.75 + 0.5 * torch.rand(chans[i], generator=g) for i in range(3)]
    shifts = [None if ws[i] is None else 0.3 * torch.randn(chans[i], generator=g) + (shift0[0], shift0[1], 0.0)[i] for i in range(3)]
    return OB16.r(x), ws, scales, shifts, stride


FUSED = "conv_mbv2_kernel"
CONVS = ("conv_igemm_kernel", "conv_pw_kernel", "conv_spw_kernel")  # what add_conv records a 1x1 layer under (a split-K pair is one record)
ROUTES = {"chain": "0", "fused": "2"}  # SYLPH_MBV2_FUSED, read at every pick_mbv2_route


def _assert_route(kernels, route, t):
    """exactly the launches of the route: ONE conv_mbv2 launch, or the chain: [expand,] depthwise, project"""
    if route == "fused":
        assert list(kernels) == [FUSED] and kernels[FUSED]["launches"] == 1, kernels
    else:
        n_conv = 1 if t == 1 else 2
        assert set(kernels) <= {DW, *CONVS} and kernels[DW]["launches"] == 1, kernels
        assert sum(kernels[k]["launches"] for k in CONVS if k in kernels) == n_conv, kernels


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("hwb", BLOCK_MAPS, ids=lambda m: f"{m[0]}x{m[1]}_B{m[2]}")
@pytest.mark.parametrize("shape", MR.BLOCK_SHAPES, ids=lambda s: "c%d_t%d_c%d_s%d" % s)
def test_block_pinned_bf16(bf16_engine, monkeypatch, shape, hwb, route):
    h, w, B = hwb
    monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[route])
    x, ws, scales, shifts, stride = _block_operands(shape, h, w, B)
    eng = bf16_engine
    eng.profile_read(), eng.conv_routes()
    y = eng.mbv2_block(x, ws, scales, shifts, stride, padded=True).cpu()
    kernels, routes = eng.profile_read()["kernels"], eng.conv_routes()
    _assert_route(kernels, route, shape[1])
    assert len(routes) == (0 if route == "fused" else 1 if shape[1] == 1 else 2), routes
    cout = shape[2]
    assert y.shape[1] == eng.mbv2_padded_channels(cout) and float(y[:, cout:].abs().max() if y.shape[1] > cout else 0.0) == 0.0
    want = MR.block_bf16(x, ws, scales, shifts, stride)
    assert want.shape[2:] == ((h - 1) // stride + 1, (w - 1) // stride + 1)
    _assert_ulps(y[:, :cout], want, f"block {shape} {h}x{w} B{B} {route}", max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.mark.parametrize("route", list(ROUTES))
def test_hidden_tensor_is_zero_padded(bf16_engine, monkeypatch, route):
    """Shifts large enough that relu6(shift) > 0 on every hidden channel, on a 5x7 map (smaller than a tile of the one-launch kernel): the
    depthwise conv pads the HIDDEN tensor with zeros, not with the expand of a zero input.  The wrong variant is more than 100 ulps away
    on the restatement."""
    monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[route])
    for shape in ((24, 6, 24, 1), (32, 6, 64, 2)):
        x, ws, scales, shifts, stride = _block_operands(shape, 5, 7, 2, shift0=(2.5, 0.5))
        shifts[0] = shifts[0].abs() + 1.0
        want = MR.block_bf16(x, ws, scales, shifts, stride)
        wrong = MR.block_bf16(x, ws, scales, shifts, stride, expand_the_padding=True)
        _, worst = _ulps(wrong, want, "rms")
        assert worst > 100.0, worst
        bf16_engine.profile_read()
        y = bf16_engine.mbv2_block(x, ws, scales, shifts, stride).cpu()
        _assert_route(bf16_engine.profile_read()["kernels"], route, shape[1])
        _assert_ulps(y, want, f"border {shape} {route}", max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", [(24, 6, 24, 1), (96, 6, 160, 2), (32, 1, 16, 1)], ids=lambda s: "c%d_t%d_c%d_s%d" % s)
def test_block_output_does_not_depend_on_batch_position(bf16_engine, monkeypatch, shape, route):
    monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[route])
    x, ws, scales, shifts, stride = _block_operands(shape, 37, 61, 3)
    x[2] = x[0]
    bf16_engine.profile_read()
    y3 = bf16_engine.mbv2_block(x, ws, scales, shifts, stride)
    _assert_route(bf16_engine.profile_read()["kernels"], route, shape[1])
    y1 = bf16_engine.mbv2_block(x[:1], ws, scales, shifts, stride)
    assert torch.equal(y3[0], y3[2]) and torch.equal(y3[0], y1[0]) and not torch.equal(y3[0], y3[1])


PAYS = {(32, 1, 16, 1), (24, 6, 24, 1), (32, 6, 32, 1)}  # pick_mbv2_route's default: the shapes of profiles/mobilenet_layers.txt where fused wins


@pytest.mark.parametrize("shape", MR.BLOCK_SHAPES, ids=lambda s: "c%d_t%d_c%d_s%d" % s)
def test_default_route_is_the_measured_one(bf16_engine, monkeypatch, shape):
    """SYLPH_MBV2_FUSED not set (= 1): one launch for the block shapes where it beat the chain, the chain for every other"""
    monkeypatch.delenv("SYLPH_MBV2_FUSED", raising=False)
    x, ws, scales, shifts, stride = _block_operands(shape, 22, 14, 2)
    bf16_engine.profile_read()
    y = bf16_engine.mbv2_block(x, ws, scales, shifts, stride).cpu()
    _assert_route(bf16_engine.profile_read()["kernels"], "fused" if shape in PAYS else "chain", shape[1])
    _assert_ulps(y, MR.block_bf16(x, ws, scales, shifts, stride), f"block {shape} default route", max_ulp=2.0, max_frac=0.03, floor="rms")


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_parity_modes_always_take_the_chain(monkeypatch, dtype):
    """SYLPH_MBV2_FUSED 2 asks for the one-launch kernel wherever it can run: that is bf16 only"""
    monkeypatch.setenv("SYLPH_MBV2_FUSED", "2")
    shape = (24, 6, 24, 1)
    x, ws, scales, shifts, stride = _block_operands(shape, 22, 14, 2)
    eng = _engine(dtype, profile=True)
    eng.profile_read()
    y = eng.mbv2_block(x, ws, scales, shifts, stride).cpu()
    _assert_route(eng.profile_read()["kernels"], "chain", shape[1])
    want = MR.block(x, ws, scales, shifts, stride)
    assert float((y - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("knob,fused,dw", [("0", 0, 17), ("1", 4, 13), ("2", 17, 0)])
def test_knob_sides_whole_bf16_network(monkeypatch, knob, fused, dw):
    """0 never launches the one-launch kernel, 2 launches it for every one of the 17 blocks in bf16; the two networks agree as closely as
    each agrees with the restatement (test_bf16_network_tracks_bf16_restatement)"""
    monkeypatch.setenv("SYLPH_MBV2_FUSED", knob)
    sd, q, *_ = _full((96, 64))
    eng = _engine("bf16", profile=True)
    eng.load_state_dict(sd)
    eng.preprocess(q)
    eng.profile_read()
    eng.backbone()
    kernels = eng.profile_read()["kernels"]
    assert kernels.get(FUSED, {"launches": 0})["launches"] == fused and kernels.get(DW, {"launches": 0})["launches"] == dw, kernels
    assert kernels[STEM]["launches"] == 1


@pytest.mark.parametrize("route", list(ROUTES))
def test_teacher_forced_bf16_network(bf16_engine, monkeypatch, route):
    """every block of the network on the bf16 restatement's input to that block, all 17 with the synthetic weights"""
    from sylph_amd import synthetic as Wt
    monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[route])
    sd = Wt.mobilenet_backbone_state_dict(0)
    x, _ = OB16.preprocess(Wt.synthetic_images(2, 96, 64, seed=9))
    inputs = []
    with torch.no_grad():
        MR.mobilenet_bf16(x, sd, inputs=inputs)
    for fi, ((cin, t, cout, stride), xin) in enumerate(zip(MR.blocks(), inputs), start=1):
        ws, ss, hs = MR.block_params(sd, fi, t)
        bf16_engine.profile_read()
        y = bf16_engine.mbv2_block(xin, ws, ss, hs, stride).cpu()
        _assert_route(bf16_engine.profile_read()["kernels"], route, t)
        _assert_ulps(y, MR.block_bf16(xin, ws, ss, hs, stride), f"features.{fi} {route}", max_ulp=2.0, max_frac=0.03, floor="rms")


# ---- whole networks --------------------------------------------------------------------------------------------------------------------
_FULL = {}


def _full(hw):
    if hw in _FULL:
        return _FULL[hw]
    from oracle import backbone as OB, head as OH
    from sylph_amd import synthetic as Wt
    sd = Wt.mobilenet_backbone_state_dict(0)
    sd.update(Wt.head_state_dict(1, num_classes=60))
    q = Wt.synthetic_images(2, hw[0], hw[1], seed=3)
    q[1] = q[1][:, :hw[0] - 10, :hw[1] - 7].contiguous()
    codes = Wt.synthetic_codes(5, seed=4, scale=3.0)
    x, sizes = OB.preprocess(q)
    with torch.no_grad():
        stages = MR.mobilenet(x, sd)
        pyr = MR.mobilenet_backbone_fpn(x, sd)
        head = OH.fcos_head(pyr, sd, codes)
    _FULL[hw] = (sd, q, codes, sizes, stages, pyr, head)
    return _FULL[hw]


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
@pytest.mark.parametrize("hw", [(64, 96), (96, 64)], ids=["64x96", "96x64"])
def test_whole_network_matches_restatement(hw, dtype):
    from oracle import decode as OD
    sd, q, codes, sizes, stages, pyr, ref_head = _full(hw)
    eng = _engine(dtype, profile=True)
    eng.load_state_dict(sd)
    assert eng.preprocess(q) == hw
    eng.backbone()
    kernels = eng.profile_read()["kernels"]
    assert kernels[STEM]["launches"] == 1 and kernels[DW]["launches"] == 17 and "stem_pool_kernel" not in kernels, kernels
    for st, ch in zip((2, 3, 4, 5), (24, 32, 96, 320)):
        a, b = eng.export_stage(st).cpu(), stages[f"res{st}"]
        assert a.shape == b.shape == (2, ch, hw[0] >> st, hw[1] >> st)
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print(f"{dtype} res{st}: max err {err:.2e} of the stage's scale")
        assert err <= 1e-3
    for l, (a, b) in enumerate(zip(eng.export_pyramid(), pyr)):
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


@pytest.mark.parametrize("route", list(ROUTES))
def test_bf16_network_tracks_bf16_restatement(monkeypatch, route):
    """A coarse end-to-end check only: the bound grows with depth (about 10 % at res5), so a mis-scaled late block could pass it; what pins
    every block to ulps is test_teacher_forced_bf16_network.  This one shows that the plan wires the blocks, buffers and stage taps together.
    A bf16 pass (stem + 17 blocks + FPN on 32 / 96 / 320-channel laterals) against the bf16 form of the restatement: both round at the
    same k = 1 + 3 * blocks stores up to a stage, each adding at most 2^-9 relative error where a value sits on a rounding boundary
    (oracle/bf16.py), so k * 2^-9 relative L2 bounds a stage; a wrong operand is O(1).  The pyramid within 5e-2 of the fp32 restatement."""
    monkeypatch.setenv("SYLPH_MBV2_FUSED", ROUTES[route])
    sd, q, codes, sizes, stages, pyr, _ = _full((96, 64))
    eng = _engine("bf16")
    eng.load_state_dict(sd)
    eng.preprocess(q)
    eng.backbone()
    x, _ = OB16.preprocess(q)
    with torch.no_grad():
        want = MR.mobilenet_bf16(x, sd)
    for st, nblocks in zip((2, 3, 4, 5), (3, 6, 13, 17)):
        got = eng.export_stage(st).cpu()
        rel = float((got.double() - want[f"res{st}"].double()).norm() / want[f"res{st}"].double().norm())
        print(f"res{st} bf16 vs bf16 restatement: relative L2 {rel:.2e}")
        assert rel <= (1 + 3 * nblocks) * 2.0 ** -9
    for l, (a, b) in enumerate(zip(eng.export_pyramid(), pyr)):
        rel = float((a.cpu().double() - b.double()).norm() / b.double().norm())
        print(f"p{l + 3}: bf16 vs fp32 restatement relative L2 {rel:.2e}")
        assert rel <= 5e-2


def test_wrong_backbone_family_names_the_keys():
    from sylph_amd import synthetic as Wt
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import Engine
    with pytest.raises(RuntimeError, match=r"MODEL\.MOBILENET.*features"):
        _engine("bf16").load_state_dict(Wt.backbone_state_dict(0, depth=18))
    with pytest.raises(RuntimeError, match=r"features.*MODEL\.MOBILENET True"):
        Engine(get_default_cfg(), dtype="bf16").load_state_dict(Wt.mobilenet_backbone_state_dict(0))
    sd = Wt.mobilenet_backbone_state_dict(0)
    sd["backbone.bottom_up.features.7.conv.3.weight"] = sd["backbone.bottom_up.features.7.conv.3.weight"][:100]
    with pytest.raises(RuntimeError, match=r"features\.7\.conv\.3\.weight.*\(192, 1, 3, 3\)"):
        _engine("f32").load_state_dict(sd)


# ---- public entry points -----------------------------------------------------------------------------------------------------------------
def test_public_entry_points_on_a_mobilenet_checkpoint(tmp_path):
    """MetaFCOSRunner's model in the support, normalisation and query run types, class_code_sets, and SylphPredictor on a MobileNetV2
    checkpoint give the engine's detections; in fp32 those equal the oracle head + decode on the restated pyramid."""
    from oracle import backbone as OB, decode as OD, head as OH
    from sylph_amd import synthetic as Wt
    from sylph_amd.data import SyntheticSupportSetLoader
    from sylph_amd.engine import Engine
    from sylph_amd.evaluation import inference_normalization, inference_on_support_set_dataset
    from sylph_amd.predictor import SylphPredictor, resize_image, resize_shortest_edge_shape
    from sylph_amd.runner import MetaFCOSRunner, create_cfg
    sd = Wt.synthetic_state_dict(0, mobilenet=True)
    r = MetaFCOSRunner()
    cfg = create_cfg(r.get_default_cfg(), "sylph://COCO-Detection/Meta-FCOS/Meta-FCOS-finetune.yaml")
    cfg.MODEL.MOBILENET = True
    model = r.build_model(cfg, dtype="f32")
    model.load_state_dict(sd)
    model.eval()
    sub = inference_on_support_set_dataset(model, SyntheticSupportSetLoader(2, 1, 128, 160, seed=5), output_dir=None)  # the support step
    sub = inference_normalization(model, sub)                                                                          # meta_learn_normalize_code
    code_dir = str(tmp_path / "codes" / "synthetic_all" / "0")
    os.makedirs(code_dir)
    for c in sub:
        c["class_code"] = {k: v.cpu() for k, v in c["class_code"].items()}
        c["class_code"]["cls_conv"] = c["class_code"]["cls_conv"] * 3.0
        torch.save(c, os.path.join(code_dir, f"{c['class_name']}.pth"))
    ckpt = str(tmp_path / "model_final.pth")
    torch.save({"model": sd}, ckpt)
    yaml = str(tmp_path / "mnv2.yaml")
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
    hip_head = [[t.cpu() for t in ts] for ts in eng.export_head()]
    want = eng.decode()[0]
    assert len(out) == want["scores"].numel() > 0
    np.testing.assert_allclose(np.sort(out.scores.cpu().numpy()), np.sort(want["scores"].cpu().numpy()), atol=1e-5)
    got = model([{"image": x, "height": nh, "width": nw}], class_code={k: v for k, v in codes.items()},
                run_type="meta_learn_test_instance")[0]["instances"]                                                   # the query step
    assert len(got) == want["scores"].numel()
    np.testing.assert_allclose(np.sort(got.scores.cpu().numpy()), np.sort(want["scores"].cpu().numpy()), atol=1e-5)
    sets = model([{"image": x, "height": nh, "width": nw}], class_code_sets=[dict(codes), dict(codes)], run_type="meta_learn_test_instance")
    for s in sets:
        inst = s[0]["instances"]
        assert len(inst) == len(got)
        np.testing.assert_allclose(np.sort(inst.scores.cpu().numpy()), np.sort(got.scores.cpu().numpy()), atol=1e-5)
    # the same detections from the oracle head and decode on the restated pyramid
    xin, sizes = OB.preprocess([x])
    cpu_codes = {k: v.cpu() for k, v in codes.items()}
    with torch.no_grad():
        ref_head = OH.fcos_head(MR.mobilenet_backbone_fpn(xin, sd), sd, cpu_codes)
    for name, hs, rs in zip(("logits", "reg", "ctrness", "iou"), hip_head, ref_head):
        for l in range(5):
            assert float((hs[l] - rs[l]).abs().max()) <= 1e-3, (name, l)
    wh = OD.detector_postprocess(OD.predict_proposals(*hip_head)[0], sizes[0], nh, nw)
    assert want["scores"].numel() == wh["scores"].numel()
    np.testing.assert_array_equal(want["pred_classes"].cpu().numpy(), wh["pred_classes"].numpy())
    np.testing.assert_allclose(want["scores"].cpu().numpy(), wh["scores"].numpy(), atol=1e-5)
    np.testing.assert_allclose(want["pred_boxes"].cpu().numpy(), wh["pred_boxes"].numpy(), atol=1e-3)
