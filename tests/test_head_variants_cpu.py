"""The float64 restatement of the FCOS head's tower variants (tests/deform_ref.py, tests/head_variants.py), checked on the host before
tests/test_head_variants_gpu.py holds the HIP head to it:

  * its two forms of the deformable conv -- explicit loops and F.grid_sample -- agree to float64 rounding in every variant, on every
    level of at least 2 x 2 (smaller maps have the loop form only);
  * with zero offset weights and saturated masks it equals oracle.head.fcos_head of the plain twin, shared tower and NORM "none" included;
  * config_from_cfg accepts every variant and maps the switches onto the C struct;
  * the codes and detection thresholds the GPU file uses give detections on every image for the restatement alone, and the thresholds
    of the fp32 comparisons sit in a gap of the restatement's class probabilities."""
import pytest
import torch

from tests import deform_ref as DR
from tests import head_variants as HV

DEFORMABLE = [v for v in HV.VARIANTS if HV.VARIANTS[v][4]]


@pytest.mark.parametrize("v", list(HV.VARIANTS))
def test_loop_and_grid_sample_forms_agree(v, monkeypatch):
    """one image (the forms do not mix images), all five levels, 5-way codes.  The restatement as the GPU file uses it (deform_conv_any:
    grid-sample form on the four levels of at least 2 x 2, loop form on the 1 x 2 map) against the loop form on every level; the plain
    variants run the same code with no deformable layer at all."""
    sd, fs, cd = HV.state_dict(v), [f[:1] for f in HV.feats()], HV.codes("n5")
    loop = HV.restate(v, sd, fs, cd, deform=DR.deform_conv_loop)
    seen, grid_form = [], DR.deform_conv_grid_sample
    monkeypatch.setattr(DR, "deform_conv_grid_sample", lambda x, *a: (seen.append(tuple(x.shape[-2:])), grid_form(x, *a))[1])
    auto = HV.restate(v, sd, fs, cd)
    assert sorted(seen) == sorted(HV.LEVELS[:4] * HV.deform_towers(v)), (v, seen)
    for t, name in enumerate(("logits", "reg", "ctr", "iou")):
        for l in range(5):
            a, g = loop[t][l], auto[t][l]
            assert float((a - g).abs().max()) <= 1e-10 * max(1.0, float(a.abs().max())), (v, name, l)
            assert bool(torch.isfinite(g).all())
        assert torch.equal(auto[t][4], loop[t][4]), (v, name)  # the 1 x 2 map: the loop form in both


@pytest.mark.parametrize("v", DEFORMABLE)
def test_zero_offsets_equal_the_plain_oracle(v):
    """the weight swap of test_deform_gpu.py::test_zero_offsets_equal_plain_tower: offsets 0, sigmoid(40) == 1 in float64"""
    from oracle import head as OH
    from sylph_amd import synthetic as Wt
    norm, share, nc, nb, _ = HV.VARIANTS[v]
    sd = HV.state_dict(v)
    plain = Wt.head_state_dict(seed=21, num_classes=60, num_share_convs=share, norm=norm, num_cls_convs=nc, num_box_convs=nb)
    for tower in ("cls_tower", "bbox_tower"):
        pre = HV.last_layer_key(v, tower)
        if pre is None:
            continue
        sd[f"{pre}.offset.weight"].zero_()
        sd[f"{pre}.offset.bias"].zero_()
        sd[f"{pre}.offset.bias"][18:] = 40.0
        plain[f"{pre}.weight"] = sd[f"{pre}.conv.weight"]
        plain[f"{pre}.bias"] = sd[f"{pre}.conv.bias"]
    fs, cd = HV.feats(), HV.codes("n5")
    got = HV.restate(v, sd, fs, cd)
    want = OH.fcos_head([f.double() for f in fs], {k: t.double() for k, t in plain.items()}, {k: t.double() for k, t in cd.items()},
                        num_cls_convs=nc, num_box_convs=nb, num_share_convs=share, norm=norm)
    assert HV.worst_rel(got, want) <= 1e-10, v
    # the swap is not vacuous: with its own offsets the variant differs from the plain twin
    assert HV.worst_rel(HV.reference(v, "n5"), want) > 1e-2, v


@pytest.mark.parametrize("v", list(HV.VARIANTS))
def test_config_accepts_the_variant(v):
    from sylph_amd.engine import config_from_cfg
    norm, share, nc, nb, dfm = HV.VARIANTS[v]
    sc = config_from_cfg(HV.cfg(v))
    assert sc.tower_deformable == int(dfm)
    assert sc.tower_norm == (0 if norm == "GN" else 1)
    assert (sc.num_share_convs, sc.num_cls_convs, sc.num_box_convs) == (share, nc, nb)
    sc3 = config_from_cfg(HV.cfg(v, **{"MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER": ["", "", 3]}))
    assert sc3.cg_code_ksize == 3 and sc3.tower_deformable == int(dfm)


@pytest.mark.parametrize("v", list(HV.VARIANTS))
def test_config_refuses_the_fused_3x3_route_on_deformable_groupnorm_towers(v, monkeypatch):
    """SYLPH_GN_COND3X3=1 sends 3x3 codes through gn_cond3x3_kernel, whose scores differ from the default route's in the last fp32 bit
    (tests/test_head_variants_gpu.py): refused where deformable towers would take it -- GroupNorm towers, 3x3 codes -- and nowhere else"""
    from sylph_amd.engine import config_from_cfg
    norm, share, nc, nb, dfm = HV.VARIANTS[v]
    k3 = {"MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER": ["", "", 3]}
    monkeypatch.setenv("SYLPH_GN_COND3X3", "1")
    assert config_from_cfg(HV.cfg(v)).cg_code_ksize == 1  # 1x1 codes never take the kernel
    if dfm and norm == "GN":
        with pytest.raises(NotImplementedError, match="SYLPH_GN_COND3X3=1 with MODEL.FCOS.USE_DEFORMABLE"):
            config_from_cfg(HV.cfg(v, **k3))
    else:
        assert config_from_cfg(HV.cfg(v, **k3)).cg_code_ksize == 3
    monkeypatch.setenv("SYLPH_GN_COND3X3", "0")
    assert config_from_cfg(HV.cfg(v, **k3)).cg_code_ksize == 3


def test_table_counts_deformable_towers():
    assert [HV.deform_towers(v) for v in HV.VARIANTS] == [2, 2, 2, 2, 1, 2, 0, 0]
    for v in DEFORMABLE:  # the synthetic checkpoint has the DFConv2d keys exactly where the table says
        sd = HV.state_dict(v)
        n = sum(1 for k in sd if k.endswith(".offset.weight"))
        assert n == HV.deform_towers(v), (v, n)
        assert not any(".share_tower." in k and ".offset." in k for k in sd)


@pytest.mark.parametrize("v", list(HV.VARIANTS))
def test_restatement_alone_detects_on_every_image(v):
    """what the GPU file relies on: with its codes the restatement gives every image detections at the default threshold (bf16
    identities) and at the thresholds of the fp32 decode comparisons, where no class probability sits within SEPARATION of the
    threshold and no two detections of an image within SEPARATION of each other (tests/head_variants.py)"""
    for name in ("n5", "n20", "n40"):
        thrs = [0.05]
        if name != "n20":
            thr, half, sep = HV.threshold(v, name)
            print(f"{v} {name}: threshold {thr:.6f}, nearest class probability {half:.2e} away, detection scores {sep:.2e} apart")
            assert 0.05 < thr < 1.0 and half >= HV.SEPARATION and sep >= HV.SEPARATION, (v, name, thr, half, sep)
            thrs.append(thr)
        for t in thrs:
            dets = HV.oracle_detections(HV.reference(v, name), t)
            for i, d in enumerate(dets):
                assert d["scores"].numel() > 0, f"{v} {name} threshold {t}: image {i} has no detection"
            if t != 0.05:
                n = [d["scores"].numel() for d in dets]
                print(f"{v} {name}: {n} detections")
                assert max(n) < 100, (v, name, n)  # below POST_NMS_TOPK_TEST: no k-th score cut
    if v in ("gn_d", "none_d"):
        for i, d in enumerate(HV.oracle_detections(HV.reference(v, "k3"), 0.05)):
            assert d["scores"].numel() > 0, f"{v} 3x3 codes: image {i} has no detection"
