"""Batch position at the headline batch: 192 images per step, as bench.py runs the C4 (R-101, 866-way) and C5 (ROI-Encoder, 337-way)
legs.  At 192 full-size images the res2 activations are 6.6e9 bytes, images 145-191 sit on per-image 64-bit bases, and the many-way
candidate buffers are 960 (image, level) segments of 1.8 M (C4) / 0.7 M (C5) slots; the fused many-way scan (logits_scan_kernel) fills
them.  Four distinct images repeated 48 times: every copy must come out BIT FOR BIT the same wherever it sits -- pyramid and
detections -- and the pyramid of images 0-3 must equal a separate 4-image run up to bf16 rounding.

One engine at a time (the C4 candidate buffers alone are ~14 GB); comparisons on the device."""
import pytest
import torch

from test_hip_parity import _cfg, _engine

pytestmark = pytest.mark.gpu

NB = 192
FIELDS = ("pred_boxes", "scores", "pred_classes", "fpn_levels", "locations", "cand_index")
C5_YAML = "sylph://LVISv1-Detection/Meta-FCOS/Meta-FCOS-ROI-Encoder-finetune.yaml"


def _headline_batch(cfg, sd, H, W, padded, nway, img_seed, code_seed):
    from sylph_amd import synthetic as Wt
    base = Wt.synthetic_images(4, H, W, seed=img_seed)
    eng = _engine("bf16", cfg)
    eng.load_state_dict(sd)
    assert eng.preprocess([base[i % 4] for i in range(NB)]) == padded
    eng.backbone()
    pyr = eng.export_pyramid()
    for lvl, p in enumerate(pyr):
        assert bool(torch.isfinite(p[0:4]).all()), f"level {lvl}: non-finite values"
        for k in range(1, NB // 4):
            assert torch.equal(p[0:4], p[4 * k:4 * k + 4]), \
                f"level {lvl}: copy {k} differs from copy 0 by {(p[0:4] - p[4 * k:4 * k + 4]).abs().max().item()}"
    small = [p[0:4].clone() for p in pyr]
    del pyr
    # bench.py's run_leg: the largest of a few code scales whose candidates fit the decode buffers (1 / 8 of a level's scores)
    eng.profile_enable(True)
    for scale in (1.5, 1.0, 0.7, 0.5):
        codes = Wt.synthetic_codes(nway, seed=code_seed, scale=scale)
        eng.profile_read()
        eng.head(codes["cls_conv"], codes["cls_bias"])
        fused = "logits_scan_kernel" in eng.profile_read()["kernels"]
        try:
            det = eng.decode()
            break
        except RuntimeError as ex:
            if "candidate capacity" not in str(ex):
                raise
    else:
        raise AssertionError("no synthetic code scale fits the candidate buffers")
    eng.profile_enable(False)
    print(f"{nway}-way at {NB} images: code scale {scale}")
    assert fused, "the fused many-way scan did not run"
    assert len(det) == NB
    for i in range(4):
        n = det[i]["scores"].numel()
        assert n > 0 and int(det[i]["pred_classes"].max()) < nway, f"image {i}: {n} detections"
    for i in range(4, NB):
        a, b = det[i], det[i % 4]
        assert a["scores"].numel() == b["scores"].numel(), f"image {i}: {a['scores'].numel()} detections, its copy {i % 4}: {b['scores'].numel()}"
        for k in FIELDS:
            assert torch.equal(a[k], b[k]), f"image {i}: {k} differs from its copy {i % 4}"
    del det
    eng.close()
    eng4 = _engine("bf16", cfg)
    eng4.load_state_dict(sd)
    eng4.preprocess(base)
    eng4.backbone()
    for lvl, (a, b) in enumerate(zip(small, eng4.export_pyramid())):
        scale = b.abs().max().item()
        assert (a - b).abs().max().item() <= 4e-2 * scale, f"level {lvl}: batch-{NB} pyramid vs batch-4 pyramid"
    eng4.close()


def test_c4_r101_866way_batch192_positions_bf16():
    """C4 geometry (bench leg c4_r101_866way): R-101, 866 classes, POST_NMS_TOPK 300, 800x1333 queries (-> 800x1344).  Code scale
    1.5 as test_c4_shape_runs_bf16_full_size, or the next smaller one if its candidates overflow the buffers (bench.py's rule)."""
    from sylph_amd import synthetic as Wt
    cfg = _cfg(**{"MODEL.RESNETS.DEPTH": 101, "MODEL.FCOS.POST_NMS_TOPK_TEST": 300})
    _headline_batch(cfg, Wt.synthetic_state_dict(0, depth=101), 800, 1333, (800, 1344), 866, img_seed=21, code_seed=22)


def test_c5_roi_encoder_337way_batch192_positions_bf16():
    """C5 geometry (bench leg c5_roi_encoder_337way): the ROI-Encoder model of Meta-FCOS-ROI-Encoder-finetune.yaml (CondConvBlock head
    with the checkpoint's Scale), its synthetic weights as bench.py builds them, 337 classes, POST_NMS_TOPK 300, 800x1200 queries
    (-> 800x1216: level widths 152 / 76 / 38 / 19 / 10).  Code scale: 1.5 or the next smaller one that fits, as bench.py chooses it
    (its C5 leg runs at 1.0)."""
    from sylph_amd import synthetic as Wt
    from sylph_amd.runner import MetaFCOSROIEncoderRunner, create_cfg
    cfg = create_cfg(MetaFCOSROIEncoderRunner().get_default_cfg(), C5_YAML, ["MODEL.META_LEARN.EVAL_SHOT", 5])
    cfg.MODEL.FCOS.POST_NMS_TOPK_TEST = 300
    sd = {}
    sd.update(Wt.backbone_state_dict(0, depth=50))
    sd.update(Wt.head_state_dict(1, num_classes=60))
    sd.update(Wt.roi_encoder_state_dict(seed=4))
    _headline_batch(cfg, sd, 800, 1200, (800, 1216), 337, img_seed=31, code_seed=32)
