"""3x3 class codes (MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER = ["", "", 3]), the parts that need no GPU: the config mapping and the C
struct, the plain torch restatements of tests/spatial_codes_ref.py against the reference's own outputs (g10_spatial_codes.npz,
tests/golden/gen_spatial_codes_golden.py) to the bound test_oracle_golden.py holds the oracle to, and the packed-row paths that must
refuse such a code by name instead of reshaping it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spatial_codes_ref as R
from oracle import decode as D
from oracle import head as H
from sylph_amd import synthetic as W
from test_oracle_golden import TOL, _checksum, _feats, _load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(cls_layer):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg.CONV_L2_NORM = True
    cg.TOWER_LAYERS = [["GN", "ReLU"], ["GN", "ReLU"]]
    cg.CLS_LAYER = cls_layer
    cg.BIAS_LAYER = ["", "", 1]
    return cfg


# ------------------------------------------------------------------------------------------------ 1: config
def test_config_maps_cls_layer_kernel_size():
    from sylph_amd.engine import config_from_cfg
    assert config_from_cfg(None).cg_code_ksize == 1  # sylph_config_default
    assert config_from_cfg(_cfg(["", "", 1])).cg_code_ksize == 1
    assert config_from_cfg(_cfg(["", "", 3])).cg_code_ksize == 3
    for k in (2, 5):  # 2 cannot run in the reference (padding 1 with an even kernel grows the map); larger sizes are not built
        with pytest.raises(NotImplementedError, match="CLS_LAYER"):
            config_from_cfg(_cfg(["", "", k]))
    for bad in (["GN", "", 3], ["", "ReLU", 3]):  # norm and activation stay as restricted as for 1x1 codes
        with pytest.raises(NotImplementedError, match="CLS_LAYER"):
            config_from_cfg(_cfg(bad))


def test_roi_encoder_keeps_1x1_codes():
    """fcos.py:524: the ROIEncoder head ignores CLS_LAYER (k_s = 1)."""
    from sylph_amd.config import get_roi_encoder_default_cfg
    from sylph_amd.engine import config_from_cfg
    cfg = get_roi_encoder_default_cfg()
    cfg.MODEL.META_LEARN.EPISODIC_LEARNING = True
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cg.CLS_LAYER = ["", "", 3]
    cg.TOKENIZER.NUM_CONV, cg.TOKENIZER.NORM = 2, "GN"
    assert config_from_cfg(cfg).cg_code_ksize == 1


# ------------------------------------------------------------------------------------------------ 2: ABI
def test_header_declares_the_field_last_and_ctypes_mirrors_it():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    body = text[text.index("typedef struct sylph_config {"):text.index("} sylph_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(1) for m in re.finditer(r"\b(?:int|float)\s+(\w+)(?:\[\d+\])?\s*;", body)]
    assert fields[-1] == "cg_code_ksize"
    assert [n for n, _ in _lib.SylphConfig._fields_] == fields
    # the mirror has the C layout: the default written through the pointer lands in the last int of the struct
    sc = _lib.SylphConfig()
    _lib.lib().sylph_config_default(ctypes.byref(sc))
    assert sc.cg_code_ksize == 1 and sc.width_per_group == 64
    assert _lib.SylphConfig.cg_code_ksize.offset + 4 == ctypes.sizeof(_lib.SylphConfig)


def test_library_exports_every_declared_symbol():
    from sylph_amd import _lib
    text = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    declared = set(re.findall(r"\b(sylph_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------ 3: the restatements against the reference
@pytest.fixture(scope="module")
def g10(golden_dir):
    return _load(golden_dir, "g10_spatial_codes.npz")


@pytest.fixture(scope="module")
def g3(golden_dir):
    return _load(golden_dir, "g3_codegen.npz")


SUPPORT = [("sup", 1), ("sup", 2), ("sup", 5), ("ws", 2), ("ws", 5), ("l2", 2), ("l2", 5)]


def _cg_sd(g10, tag):
    sd = W.codegen_state_dict(seed=2, weight_scale_layers=tag == "ws")
    assert abs(_checksum(sd, "code_generator") - float(g10[f"{tag}_weights_checksum"])) < 1e-3
    return sd


def test_pool_bins_are_torchs():
    assert R.pool_bins(7, 3) == [(0, 3), (2, 5), (4, 7)]  # overlapping, nine positions per 2-D bin
    x = torch.randn(2, 5, 7, 7, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(R.adaptive_pool(x, 3), torch.nn.functional.adaptive_avg_pool2d(x, (3, 3)), atol=1e-6, rtol=0)
    assert torch.allclose(R.adaptive_pool(x, 1), x.mean(dim=(2, 3), keepdim=True), atol=1e-6, rtol=0)


@pytest.mark.parametrize("tag,S", SUPPORT)
def test_support_codes_match_reference(g10, g3, tag, S):
    sd = _cg_sd(g10, tag)
    code = R.code_generator(_feats(g3, f"s{S}_feat"), torch.from_numpy(g3[f"s{S}_boxes"]), sd, bias_l2_norm=tag == "l2",
                            has_weight_layer=tag == "ws", has_scale_layer=tag == "ws")
    assert tuple(code["cls_conv"].shape) == (1, 256, 3, 3)
    for k, v in code.items():
        np.testing.assert_allclose(v.numpy(), g10[f"{tag}_s{S}_{k}"], atol=TOL, rtol=TOL)


@pytest.mark.parametrize("tag,S", SUPPORT)
def test_normalised_codes_match_reference(g10, tag, S):
    sd = _cg_sd(g10, tag)
    wn = torch.from_numpy(g10[f"{tag}_s{S}_cls_weight_norm"]) if tag == "ws" else None
    conv, bias = R.normalize_code(torch.from_numpy(g10[f"{tag}_s{S}_cls_conv"]), torch.from_numpy(g10[f"{tag}_s{S}_cls_bias"]), sd, wn)
    np.testing.assert_allclose(conv.numpy(), g10[f"{tag}_s{S}_norm_cls_conv"], atol=TOL, rtol=TOL)
    np.testing.assert_allclose(bias.numpy(), g10[f"{tag}_s{S}_norm_cls_bias"], atol=TOL, rtol=TOL)
    if tag != "ws":  # every tap's L2 norm over the channels is conv_scale
        scale = float(sd[f"{R.CG_PREFIX}.conv_scale.scale"])
        assert (conv.norm(dim=1) - scale).abs().max() < 1e-4


def test_formatted_codes_match_reference(g10):
    recs = [{"support_set_target": t, "class_code": {"cls_conv": torch.from_numpy(g10[f"sup_s{S}_norm_cls_conv"]),
                                                      "cls_bias": torch.from_numpy(g10[f"sup_s{S}_norm_cls_bias"])}}
            for t, S in ((2, 5), (0, 1), (1, 2))]
    fm = R.format_codes(recs)
    assert tuple(fm["cls_conv"].shape) == (3, 256, 3, 3) and tuple(fm["cls_bias"].shape) == (3,)
    np.testing.assert_array_equal(fm["cls_conv"].numpy(), g10["sup_fmt_cls_conv"])
    np.testing.assert_array_equal(fm["cls_bias"].numpy(), g10["sup_fmt_cls_bias"])
    # the package's own formatter (unchanged) carries the spatial axes through
    from sylph_amd.evaluation import format_class_codes_shared
    mine = format_class_codes_shared([dict(r, class_name="c") for r in recs], "cpu")
    np.testing.assert_array_equal(mine["cls_conv"].numpy(), g10["sup_fmt_cls_conv"])
    np.testing.assert_array_equal(mine["cls_bias"].numpy(), g10["sup_fmt_cls_bias"])


@pytest.fixture(scope="module")
def head_sd(g10):
    sd = W.head_state_dict(seed=1, num_classes=60)
    assert abs(_checksum(sd, "proposal_generator") - float(g10["head_weights_checksum"])) < 1e-3
    return sd


@pytest.fixture(scope="module")
def cls_towers(golden_dir, head_sd):
    """the cls tower's output on g1's pyramid: it does not depend on the codes"""
    g1 = _load(golden_dir, "g1_head_decode.npz")
    return [H.tower(f, head_sd, f"{H.HEAD_PREFIX}.cls_tower") for f in _feats(g1)]


@pytest.mark.parametrize("tag", ["n1", "n5", "n20", "tap9"])
def test_head_logits_match_reference(g10, cls_towers, tag):
    w, b = torch.from_numpy(g10[f"{tag}_cls_conv"]), torch.from_numpy(g10[f"{tag}_cls_bias"])
    for l, t in enumerate(cls_towers):
        np.testing.assert_allclose(R.cond_conv(t, w, b).numpy(), g10[f"{tag}_logits{l}"], atol=TOL, rtol=TOL)


def test_one_tap_codes_see_orientation(g10, cls_towers):
    """the adversarial set: a swapped ky / kx or a convolution (flipped kernel) moves whole classes far outside the bound"""
    w, b = torch.from_numpy(g10["tap9_cls_conv"]), torch.from_numpy(g10["tap9_cls_bias"])
    want = g10["tap9_logits0"]
    for wrong in (w.transpose(2, 3), w.flip(2, 3)):
        got = R.cond_conv(cls_towers[0], wrong.contiguous(), b).numpy()
        assert np.abs(got - want).max() > 1000 * TOL * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("tag", ["n5", "tap9"])
def test_decode_matches_reference(g10, tag):
    logits = [torch.from_numpy(g10[f"{tag}_logits{l}"]) for l in range(5)]
    regs, ctrs, ious = ([torch.from_numpy(g10[f"{n}{l}"]) for l in range(5)] for n in ("reg", "ctr", "iou"))
    props = D.predict_proposals(logits, regs, ctrs, ious, pre_nms_thresh=0.05)
    for i, p in enumerate(props):
        pre = f"{tag}_img{i}"
        assert p["scores"].numel() == int(g10[f"{tag}_count"][i]) > 0
        np.testing.assert_array_equal(p["pred_classes"].numpy(), g10[f"{pre}_pred_classes"])
        np.testing.assert_array_equal(p["fpn_levels"].numpy(), g10[f"{pre}_fpn_levels"])
        np.testing.assert_array_equal(p["locations"].numpy(), g10[f"{pre}_locations"])
        np.testing.assert_allclose(p["scores"].numpy(), g10[f"{pre}_scores"], atol=1e-6, rtol=1e-6)
        np.testing.assert_allclose(p["pred_boxes"].numpy(), g10[f"{pre}_pred_boxes"], atol=1e-4, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 4: the packed 280-float row paths
def _record(k):
    return {"support_set_target": 0, "class_name": "c", "class_code": {"cls_conv": torch.ones(1, 256, k, k), "cls_bias": torch.zeros(1, 1, 1, 1)}}


def test_packed_row_paths_refuse_3x3_codes_by_name():
    from sylph_amd import distributed as Dist
    from sylph_amd.runner import _rows_from_codes, reduce_class_code
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        _rows_from_codes([_record(3)], torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        Dist.pack_codes(torch.ones(1, 256, 3, 3), torch.zeros(1), [0])
    with pytest.raises(NotImplementedError, match="CLS_LAYER"):
        reduce_class_code([_record(3), _record(3)])
    # 1x1 records pack as before
    assert tuple(_rows_from_codes([_record(1)], torch.device("cpu")).shape) == (1, Dist.ROW)
    assert len(reduce_class_code([_record(1), _record(1)])) == 1
