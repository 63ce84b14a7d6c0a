"""MobileNetV2 backbones (MODEL.MOBILENET True, AdelaiDet's build_mnv2_backbone behind build_fcos_resnet_fpn_backbone) on the host: the
config key maps onto the C struct and the two bottom-up variants AdelaiDet tests first still refuse, the synthetic checkpoint has the
tonylins key set and shapes, the test-side restatement (tests/mobilenet_ref.py) equals an independent implementation (transformers'
MobileNetV2Model), the synthetic weights give both clamps of every ReLU6 real work, the bf16 form tracks the fp32 form, and a
checkpoint with backbone.bottom_up.features.* keys passes through the readers."""
import pickle

import pytest
import torch

from tests import mobilenet_ref as MR


def _cfg(mobilenet=True, anti_alias=False, deform_interval=1, **resnets):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cfg.MODEL.MOBILENET = mobilenet
    cfg.MODEL.BACKBONE.ANTI_ALIAS = anti_alias
    cfg.MODEL.RESNETS.DEFORM_INTERVAL = deform_interval
    for k, v in resnets.items():
        cfg.MODEL.RESNETS[k] = v
    return cfg


def test_config_maps_mobilenet():
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import config_from_cfg
    assert config_from_cfg(get_default_cfg()).mobilenet == 0
    sc = config_from_cfg(_cfg())
    assert sc.mobilenet == 1
    # the FPN, head and code-generator settings are what the default config gives
    base = config_from_cfg(get_default_cfg())
    for name, _ in type(sc)._fields_:
        if name not in ("mobilenet", "strides", "pixel_mean", "pixel_std"):
            assert getattr(sc, name) == getattr(base, name), name
    assert list(sc.strides) == list(base.strides)


def test_mobilenet_does_not_read_resnet_keys():
    """RESNETS.* keys that refuse for a ResNet are not read for this backbone (AdelaiDet's build_mnv2_backbone reads none of them)"""
    from sylph_amd.engine import config_from_cfg
    sc = config_from_cfg(_cfg(DEPTH=26, RES2_OUT_CHANNELS=128, NUM_GROUPS=3, RES5_DILATION=2))
    assert sc.mobilenet == 1 and (sc.num_groups, sc.width_per_group) == (1, 64)
    with pytest.raises(NotImplementedError, match="DEPTH"):
        config_from_cfg(_cfg(mobilenet=False, DEPTH=26))


@pytest.mark.parametrize("mobilenet", [False, True])
@pytest.mark.parametrize("kw,match", [({"anti_alias": True}, r"MODEL\.BACKBONE\.ANTI_ALIAS"),
                                      ({"deform_interval": 3}, r"MODEL\.RESNETS\.DEFORM_INTERVAL"),
                                      ({"anti_alias": True, "deform_interval": 2}, r"MODEL\.BACKBONE\.ANTI_ALIAS")])
def test_config_refuses_the_other_bottom_up_variants(mobilenet, kw, match):
    """AdelaiDet tests ANTI_ALIAS, then DEFORM_INTERVAL > 1, then MOBILENET: the first two refuse by name, with MOBILENET too"""
    from sylph_amd.engine import config_from_cfg
    with pytest.raises(NotImplementedError, match=match):
        config_from_cfg(_cfg(mobilenet=mobilenet, **kw))
    assert config_from_cfg(_cfg(mobilenet=mobilenet, deform_interval=1)).mobilenet == int(mobilenet)


def test_ctypes_mirror_matches_the_header():
    """the header and the ctypes mirror declare the same fields in the same order; `mobilenet` sits right in front of cg_code_ksize, which
    tests/test_spatial_codes_cpu.py pins as the last field"""
    import os
    import re
    from sylph_amd._lib import SylphConfig
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "sylph_hip.h")).read()
    body = text[text.index("typedef struct sylph_config {"):text.index("} sylph_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(?:int|float)\s+(\w+)(?:\[\d+\])?\s*;", body)
    assert names == [n for n, _ in SylphConfig._fields_]
    assert names[-2:] == ["mobilenet", "cg_code_ksize"]


def test_synthetic_dict_has_the_tonylins_keys_and_shapes():
    from sylph_amd import synthetic as W
    sd = W.mobilenet_backbone_state_dict(0)
    want = MR.expected_keys()
    for stage, c in ((3, 32), (4, 96), (5, 320)):
        want.update({f"backbone.fpn_lateral{stage}.weight": (256, c, 1, 1), f"backbone.fpn_lateral{stage}.bias": (256,),
                     f"backbone.fpn_output{stage}.weight": (256, 256, 3, 3), f"backbone.fpn_output{stage}.bias": (256,)})
    for n in ("p6", "p7"):
        want.update({f"backbone.top_block.{n}.weight": (256, 256, 3, 3), f"backbone.top_block.{n}.bias": (256,)})
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == s for k, s in want.items())
    assert len(MR.blocks()) == 17 and len(MR.BLOCK_SHAPES) == 12
    assert MR.BLOCK_SHAPES == [(32, 1, 16, 1), (16, 6, 24, 2), (24, 6, 24, 1), (24, 6, 32, 2), (32, 6, 32, 1), (32, 6, 64, 2), (64, 6, 64, 1),
                               (64, 6, 96, 1), (96, 6, 96, 1), (96, 6, 160, 2), (160, 6, 160, 1), (160, 6, 320, 1)]
    assert W.mobilenet_v2_blocks() == MR.blocks()
    # no trailing 1x1 to 1280, no classifier
    assert not any(k.startswith("backbone.bottom_up.features.18") or "classifier" in k for k in sd)
    # the whole-model dict carries them, and every key of the default dicts is bit-stable
    full = W.synthetic_state_dict(0, mobilenet=True)
    assert all(torch.equal(full[k], v) for k, v in sd.items()) and not any(".stem." in k or ".res2." in k for k in full)
    r50, head = W.synthetic_state_dict(0), W.head_state_dict(1, 60)
    assert not any(".features." in k for k in r50)
    assert all(torch.equal(full[k], v) for k, v in head.items()) and all(torch.equal(r50[k], v) for k, v in head.items())
    g = torch.Generator().manual_seed(0)
    assert torch.equal(r50["backbone.bottom_up.stem.conv1.weight"], torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5 / 64.0)


def _hf_mobilenet(sd):
    """transformers' MobileNetV2Model loaded with the tonylins-named weights (BatchNorm2d in eval mode = FrozenBN)"""
    from transformers import MobileNetV2Config, MobileNetV2Model
    m = MobileNetV2Model(MobileNetV2Config(tf_padding=False, layer_norm_eps=1e-5), add_pooling_layer=False).eval()
    used = set()

    def put(layer, wkey, bnkey):
        with torch.no_grad():
            assert layer.convolution.weight.shape == sd[wkey + ".weight"].shape, wkey
            layer.convolution.weight.copy_(sd[wkey + ".weight"])
            used.add(wkey + ".weight")
            for k in ("weight", "bias", "running_mean", "running_var"):
                getattr(layer.normalization, k).copy_(sd[f"{bnkey}.{k}"])
                used.add(f"{bnkey}.{k}")
        assert abs(layer.normalization.eps - 1e-5) < 1e-12 and layer.convolution.bias is None

    p = MR.PREFIX
    put(m.conv_stem.first_conv, f"{p}.0.0", f"{p}.0.1")
    put(m.conv_stem.conv_3x3, f"{p}.1.conv.0", f"{p}.1.conv.1")
    put(m.conv_stem.reduce_1x1, f"{p}.1.conv.3", f"{p}.1.conv.4")
    assert len(m.layer) == 16
    for i, layer in enumerate(m.layer):
        q = f"{p}.{i + 2}.conv"
        put(layer.expand_1x1, f"{q}.0", f"{q}.1")
        put(layer.conv_3x3, f"{q}.3", f"{q}.4")
        put(layer.reduce_1x1, f"{q}.6", f"{q}.7")
    assert used == set(MR.expected_keys())
    return m


def test_restatement_equals_transformers_mobilenet_v2():
    pytest.importorskip("transformers")
    from sylph_amd import synthetic as W
    sd = W.mobilenet_backbone_state_dict(0)
    x = 60.0 * torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        hs = _hf_mobilenet(sd)(x, output_hidden_states=True).hidden_states
        got = MR.mobilenet(x, sd)
    for si, (idx, ch) in enumerate(zip((1, 4, 11, 15), (24, 32, 96, 320))):
        a, b = got[f"res{si + 2}"], hs[idx]
        assert a.shape == b.shape == (1, ch, 16 >> si, 24 >> si)
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"MobileNetV2 res{si + 2}: max error {err:.2e} of the stage's maximum")
        assert err <= 1e-5


@pytest.mark.parametrize("seed", [0, 1])
def test_synthetic_weights_work_both_clamps_of_every_relu6(seed):
    """on the fp32 restatement of a 64x96 image: after EACH ReLU6 of every block (and the stem's) 1-60 % of the values sit at 6 and
    10-90 % at 0; otherwise the GPU tests would not exercise the clamps"""
    from oracle import backbone as OB
    from sylph_amd import synthetic as W
    sd = W.mobilenet_backbone_state_dict(seed)
    x, _ = OB.preprocess(W.synthetic_images(1, 64, 96, seed=3))
    hidden = []
    with torch.no_grad():
        MR.mobilenet(x, sd, hidden=hidden)
        hidden.append([MR.stem(x, sd)])
    assert len(hidden) == 18 and [len(h) for h in hidden[:17]] == [1] + [2] * 16
    for fi, hb in enumerate(hidden, start=1):
        for j, h in enumerate(hb):
            at6, at0 = float((h == 6).float().mean()), float((h == 0).float().mean())
            print(f"features.{fi % 18} ReLU6 {j}: {100 * at6:.1f} % at 6, {100 * at0:.1f} % at 0")
            assert 0.01 <= at6 <= 0.60 and 0.10 <= at0 <= 0.90, (fi, j, at6, at0)


def test_bf16_form_tracks_fp32_form():
    from oracle import backbone as OB
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as W
    sd = W.mobilenet_backbone_state_dict(0)
    x, _ = OB.preprocess(W.synthetic_images(1, 64, 96, seed=5))
    with torch.no_grad():
        ref = MR.mobilenet_backbone_fpn(x, sd)
        got = MR.mobilenet_backbone_fpn_bf16(OB16.r(x), sd)
    for l, (a, b) in enumerate(zip(got, ref)):
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"MobileNetV2 p{l + 3}: bf16 form vs fp32 form relative L2 {rel:.2e}")
        assert a.shape == b.shape and rel <= 5e-2


def test_bf16_block_rounds_each_launch_and_the_wrong_border_differs():
    """the bf16 block form returns bf16 values and differs from the exact block by roundings only; the variant that expands the zero
    padding is far away (the border case of the GPU tests cannot be vacuous)"""
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as W
    sd = W.mobilenet_backbone_state_dict(1)
    g = torch.Generator().manual_seed(5)
    for fi, (cin, t, cout, stride) in ((1, MR.blocks()[0]), (3, MR.blocks()[2]), (4, MR.blocks()[3])):
        x = OB16.r(torch.randn(2, cin, 13, 11, generator=g).clamp(0, 6) if t == 1 else torch.randn(2, cin, 13, 11, generator=g))
        ws, ss, hs = MR.block_params(sd, fi, t)
        got = MR.block_bf16(x, ws, ss, hs, stride)
        exact = MR.block(x.double(), ws, ss, hs, stride)
        assert torch.equal(got, OB16.r(got)) and got.shape == exact.shape
        assert float((got.double() - exact).abs().max()) <= 0.03 * float(exact.abs().max())
        if t != 1:
            wrong = MR.block_bf16(x, ws, ss, hs, stride, expand_the_padding=True)
            assert wrong.shape == got.shape and torch.equal(wrong[:, :, 2:-2, 2:-2], got[:, :, 2:-2, 2:-2])
            assert float((wrong - got).abs().max()) > 0.1 * float(got.abs().max())


@pytest.mark.parametrize("kind", ["pkl", "pth"])
def test_mobilenet_checkpoint_round_trips(tmp_path, kind):
    from sylph_amd import synthetic as W
    from sylph_amd.checkpoint import load_checkpoint_file
    sd = W.synthetic_state_dict(0, mobilenet=True)
    path = str(tmp_path / f"model_final.{kind}")
    if kind == "pkl":
        with open(path, "wb") as f:
            pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "test"}, f)
    else:
        torch.save({"model": sd}, path)
    loaded = load_checkpoint_file(path)
    assert set(loaded) == set(sd)
    assert all(torch.equal(loaded[k], v) for k, v in sd.items())
    assert tuple(loaded["backbone.bottom_up.features.17.conv.6.weight"].shape) == (320, 960, 1, 1)
