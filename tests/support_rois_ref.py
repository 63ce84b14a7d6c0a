"""Gather-and-loop restatement of the ROI-list support path: ONE oracle call per segment.

A ROI list names R (image, box) pairs over a batch and cuts them into consecutive segments; segment j is, by definition, the reference
called on a support set of seg_len[j] shots whose shot i is the pyramid of the segment's i-th ROI's image with that ROI's box.  So per
segment: index_select the pyramid by the segment's roi_image entries (an image used k times appears k times), then the oracle of the
one-class call (oracle.codegen.code_generator / oracle.roi_encoder.roi_encoder).  Nothing is shared between segments."""
from typing import Dict, List, Sequence

import torch


def gather_segment(features: List[torch.Tensor], roi_image: Sequence[int], r0: int, n: int) -> List[torch.Tensor]:
    """The pyramid of the n shots of the segment that starts at ROI r0: level l -> (n, C, h_l, w_l)."""
    sel = torch.as_tensor(list(roi_image[r0:r0 + n]), dtype=torch.int64)
    return [f.index_select(0, sel) for f in features]


def segment_code_dicts(kind: str, features: List[torch.Tensor], boxes: torch.Tensor, roi_image: Sequence[int], seg_len: Sequence[int],
                       sd, **kw) -> List[Dict[str, torch.Tensor]]:
    """kind "roienc": oracle.roi_encoder; anything else: oracle.codegen (kw: code_from_roi_features' switches, strides)."""
    from oracle import codegen as CG, roi_encoder as RE
    assert sum(int(n) for n in seg_len) == len(roi_image) == boxes.shape[0]
    out, r0 = [], 0
    for n in seg_len:
        n = int(n)
        feats = gather_segment(features, roi_image, r0, n)
        if kind == "roienc":
            out.append(RE.roi_encoder(feats, boxes[r0:r0 + n], sd, num_shots=n, **kw))
        else:
            out.append(CG.code_generator(feats, boxes[r0:r0 + n], sd, **kw))
        r0 += n
    return out


def segment_codes(kind: str, features, boxes, roi_image, seg_len, sd, **kw) -> torch.Tensor:
    """-> (n_seg, 257): cls_conv ++ cls_bias per segment, the layout of Engine.codegen_rois."""
    ds = segment_code_dicts(kind, features, boxes, roi_image, seg_len, sd, **kw)
    return torch.stack([torch.cat([d["cls_conv"].reshape(-1), d["cls_bias"].reshape(-1)]) for d in ds])
