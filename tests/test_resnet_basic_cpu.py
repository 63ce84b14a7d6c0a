"""ResNet-18 / ResNet-34 backbones (MODEL.RESNETS.DEPTH 18 | 34, detectron2 BasicBlock) on the host: the config keys map onto the C
struct and every other combination still raises, the synthetic checkpoints have detectron2's key set and shapes, the test-side
restatement (tests/basic_ref.py) equals an independent implementation (transformers' ResNetModel with basic layers), its bf16 form
tracks its fp32 form, and a detectron2-named backbone pickle loads."""
import pickle

import pytest
import torch

from tests import basic_ref as BR


def _cfg(depth, res2_out=64, **resnets):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    r = cfg.MODEL.RESNETS
    r.DEPTH, r.RES2_OUT_CHANNELS = depth, res2_out
    for k, v in resnets.items():
        r[k] = v
    return cfg


@pytest.mark.parametrize("depth", [18, 34])
@pytest.mark.parametrize("stride_in_1x1", [False, True])
def test_config_maps_basic_depths(depth, stride_in_1x1):
    from sylph_amd.engine import config_from_cfg
    sc = config_from_cfg(_cfg(depth, STRIDE_IN_1X1=stride_in_1x1))  # STRIDE_IN_1X1 is ignored for BasicBlock, as in detectron2
    assert (sc.resnet_depth, sc.num_groups, sc.width_per_group) == (depth, 1, 64)


@pytest.mark.parametrize("depth,res2_out,extra,match", [
    (18, 256, {}, "RES2_OUT_CHANNELS"),
    (34, 256, {}, "RES2_OUT_CHANNELS"),
    (50, 64, {}, "RES2_OUT_CHANNELS"),
    (101, 64, {}, "RES2_OUT_CHANNELS"),
    (18, 128, {}, "RES2_OUT_CHANNELS"),
    (18, 64, {"NUM_GROUPS": 32, "WIDTH_PER_GROUP": 8}, "DEPTH 18: ResNeXt needs DEPTH 50, 101 or 152"),
    (34, 64, {"WIDTH_PER_GROUP": 32}, "DEPTH 34: ResNeXt needs DEPTH 50, 101 or 152"),
    (18, 64, {"DEFORM_ON_PER_STAGE": [False, True, True, True]}, "DEFORM_ON_PER_STAGE"),
    (34, 64, {"RES5_DILATION": 2}, "RES5_DILATION"),
    (26, 64, {}, "DEPTH"),
    (200, 256, {}, "DEPTH"),
])
def test_config_refuses_other_combinations(depth, res2_out, extra, match):
    from sylph_amd.engine import config_from_cfg
    with pytest.raises(NotImplementedError, match=match):
        config_from_cfg(_cfg(depth, res2_out, **extra))


def test_bottleneck_depths_keep_their_mapping():
    from sylph_amd.config import get_default_cfg
    from sylph_amd.engine import config_from_cfg
    sc = config_from_cfg(get_default_cfg())
    assert (sc.resnet_depth, sc.num_groups, sc.width_per_group, sc.stride_in_1x1) == (50, 1, 64, 1)


@pytest.mark.parametrize("depth", [18, 34])
def test_synthetic_basic_dicts_have_detectron2_keys_and_shapes(depth):
    from sylph_amd import synthetic as W
    sd = W.backbone_state_dict(0, depth=depth)
    bn = ("weight", "bias", "running_mean", "running_var")
    want = {"backbone.bottom_up.stem.conv1.weight": (64, 3, 7, 7)}
    want.update({f"backbone.bottom_up.stem.conv1.norm.{k}": (64,) for k in bn})
    cin = 64
    for si, nb in enumerate(BR.STAGE_BLOCKS[depth]):
        cout = 64 << si
        for bi in range(nb):
            q = f"backbone.bottom_up.res{si + 2}.{bi}"
            convs = {"conv1": (cout, cin, 3, 3), "conv2": (cout, cout, 3, 3)}
            if cin != cout:
                convs["shortcut"] = (cout, cin, 1, 1)
            for name, shape in convs.items():
                want[f"{q}.{name}.weight"] = shape
                want.update({f"{q}.{name}.norm.{k}": (cout,) for k in bn})
            cin = cout
    for stage, c in ((3, 128), (4, 256), (5, 512)):
        want.update({f"backbone.fpn_lateral{stage}.weight": (256, c, 1, 1), f"backbone.fpn_lateral{stage}.bias": (256,),
                     f"backbone.fpn_output{stage}.weight": (256, 256, 3, 3), f"backbone.fpn_output{stage}.bias": (256,)})
    for n in ("p6", "p7"):
        want.update({f"backbone.top_block.{n}.weight": (256, 256, 3, 3), f"backbone.top_block.{n}.bias": (256,)})
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == s for k, s in want.items())
    assert not any(".conv3." in k for k in sd) and not any(k.startswith("backbone.bottom_up.res2.0.shortcut") for k in sd)
    assert sum(k.endswith("shortcut.weight") for k in sd) == 3
    # the whole-model dict carries them too, and the default dicts are what they were
    full = W.synthetic_state_dict(0, depth=depth)
    assert torch.equal(full["backbone.bottom_up.res5.1.conv2.weight"], sd["backbone.bottom_up.res5.1.conv2.weight"])
    assert tuple(W.backbone_state_dict(0)["backbone.bottom_up.res2.0.conv1.weight"].shape) == (64, 64, 1, 1)


def _hf_resnet(sd, depth):
    """transformers' ResNetModel with basic layers, loaded with the detectron2-named weights (BatchNorm2d in eval mode = FrozenBN)."""
    from transformers import ResNetConfig, ResNetModel
    cfg = ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[64, 128, 256, 512], depths=list(BR.STAGE_BLOCKS[depth]),
                       layer_type="basic", hidden_act="relu", downsample_in_first_stage=False)
    m = ResNetModel(cfg).eval()

    def put(conv_layer, name):
        with torch.no_grad():
            conv_layer.convolution.weight.copy_(sd[name + ".weight"])
            for k in ("weight", "bias", "running_mean", "running_var"):
                getattr(conv_layer.normalization, k).copy_(sd[f"{name}.norm.{k}"])
        assert abs(conv_layer.normalization.eps - 1e-5) < 1e-12

    p = "backbone.bottom_up"
    put(m.embedder.embedder, f"{p}.stem.conv1")
    n_sc = 0
    for si, stage in enumerate(m.encoder.stages):
        for bi, layer in enumerate(stage.layers):
            q = f"{p}.res{si + 2}.{bi}"
            put(layer.layer[0], q + ".conv1")
            put(layer.layer[1], q + ".conv2")
            if hasattr(layer.shortcut, "convolution"):
                put(layer.shortcut, q + ".shortcut")
                n_sc += 1
            else:
                assert q + ".shortcut.weight" not in sd
    assert n_sc == 3
    return m


@pytest.mark.parametrize("depth", [18, 34])
def test_restatement_equals_transformers_basic_resnet(depth):
    pytest.importorskip("transformers")
    from sylph_amd import synthetic as W
    sd = W.backbone_state_dict(0, depth=depth)
    x = torch.randn(1, 3, 256, 320, generator=torch.Generator().manual_seed(depth))
    with torch.no_grad():
        hs = _hf_resnet(sd, depth)(x, output_hidden_states=True).hidden_states
        got = BR.resnet(x, sd, depth)
    assert len(hs) == 5
    for si in range(4):
        a, b = got[f"res{si + 2}"], hs[si + 1]
        assert a.shape == b.shape == (1, 64 << si, 64 >> si, 80 >> si)
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"R-{depth} res{si + 2}: max error {err:.2e} of the stage's maximum")
        assert err <= 1e-5


@pytest.mark.parametrize("depth", [18, 34])
def test_bf16_form_tracks_fp32_form(depth):
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as W
    sd = W.backbone_state_dict(0, depth=depth)
    x = torch.randn(1, 3, 256, 320, generator=torch.Generator().manual_seed(depth + 1))
    with torch.no_grad():
        ref = BR.basic_backbone_fpn(x, sd, depth)
        got = BR.basic_backbone_fpn_bf16(OB16.r(x), sd, depth)
    for l, (a, b) in enumerate(zip(got, ref)):
        rel = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"R-{depth} p{l + 3}: bf16 form vs fp32 form relative L2 {rel:.2e}")
        assert a.shape == b.shape and rel <= 5e-2


def test_bf16_block_rounds_each_launch():
    """the bf16 block form: every value it returns is bf16-representable, and it differs from the exact block by roundings only"""
    from oracle import bf16 as OB16
    from sylph_amd import synthetic as W
    sd = W.backbone_state_dict(1, depth=18)
    g = torch.Generator().manual_seed(5)
    for q, cin, stride, has_sc in (("backbone.bottom_up.res2.1", 64, 1, False), ("backbone.bottom_up.res3.0", 64, 2, True)):
        x = OB16.r(torch.relu(torch.randn(2, cin, 13, 11, generator=g)))
        ws, ss, hs = BR.block_params(sd, q, has_sc)
        got = BR.basic_block_bf16(x, ws, ss, hs, stride)
        exact = BR.basic_block(x.double(), {k: v.double() for k, v in sd.items()}, q, stride, has_sc)
        assert torch.equal(got, OB16.r(got)) and got.shape == exact.shape
        assert float((got.double() - exact).abs().max()) <= 0.03 * float(exact.abs().max())


@pytest.mark.parametrize("prefix", ["", "backbone.bottom_up."])
def test_detectron2_named_r18_pickle_round_trips(tmp_path, prefix):
    from sylph_amd import synthetic as W
    from sylph_amd.checkpoint import load_checkpoint_file
    sd = W.backbone_state_dict(0, depth=18)
    bu = {k[len("backbone.bottom_up."):]: v for k, v in sd.items() if k.startswith("backbone.bottom_up.")}
    path = str(tmp_path / "R-18.pkl")
    with open(path, "wb") as f:
        pickle.dump({"model": {prefix + k: v.numpy() for k, v in bu.items()}, "__author__": "test", "matching_heuristics": True}, f)
    loaded = load_checkpoint_file(path)
    assert set(loaded) == {"backbone.bottom_up." + k for k in bu}
    assert all(torch.equal(loaded["backbone.bottom_up." + k], v) for k, v in bu.items())
    assert tuple(loaded["backbone.bottom_up.res3.0.shortcut.weight"].shape) == (128, 64, 1, 1)
    assert "backbone.bottom_up.res2.0.shortcut.weight" not in loaded
