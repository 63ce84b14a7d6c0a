"""Query VIEWS, host side: the planners of test-time augmentation and tiled inference.

A view is a dict {"crop": (x0, y0, cw, ch), "size": (new_h, new_w), "flip": bool} of one source image: the crop, resized to `size`
(PIL BILINEAR), mirrored afterwards when `flip`.  Engine.preprocess_views cuts the views of a step out of sources resident on the
device (a "source" key names the source of each view there), the per-view decode runs with the crop size as output size, and
Engine.merge_views (Engine.merge_views_large for a source of more than MERGE_POOL_CAP rows: merge_route) pools the views of a source
under one class-wise NMS, in the coordinates of the source.  Nothing here touches the GPU."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

DEFAULT_MAX_BATCH = 192  # views per step: the batch the benchmark runs at
# rows of one source (max_in x its views) that Engine.merge_views pools on chip (csrc/kernels.h); Engine.merge_views_large goes beyond
MERGE_POOL_CAP = 4096


def resize_shortest_edge_shape(h: int, w: int, size: int, max_size: int) -> Tuple[int, int]:
    """detectron2 ResizeShortestEdge.get_output_shape (sylph/predictor.py:117-120 builds it with
    [MIN_SIZE_TEST, MIN_SIZE_TEST], MAX_SIZE_TEST)."""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        s = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * s, neww * s
    return int(newh + 0.5), int(neww + 0.5)


def make_view(crop: Sequence[int], size: Sequence[int], flip: bool = False) -> Dict:
    x0, y0, cw, ch = (int(v) for v in crop)
    return {"crop": (x0, y0, cw, ch), "size": (int(size[0]), int(size[1])), "flip": bool(flip)}


def check_views(views: Sequence[Dict], h: int, w: int, what: str = "views") -> List[Dict]:
    """The view dicts of an (h, w) source, normalised; a crop that leaves the source or an empty size raises ValueError by name."""
    out = []
    if len(views) == 0:
        raise ValueError(f"{what}: the view list is empty")
    for i, v in enumerate(views):
        x0, y0, cw, ch = (int(t) for t in v["crop"])
        nh, nw = (int(t) for t in v["size"])
        if cw <= 0 or ch <= 0 or nh <= 0 or nw <= 0:
            raise ValueError(f"{what}[{i}]: crop {cw} x {ch} -> {nw} x {nh}: sizes must be positive")
        if x0 < 0 or y0 < 0 or x0 + cw > w or y0 + ch > h:
            raise ValueError(f"{what}[{i}]: crop ({x0}, {y0}) + {cw} x {ch} leaves its {w} x {h} source")
        out.append(make_view((x0, y0, cw, ch), (nh, nw), bool(v.get("flip", False))))
    return out


def tta_views(h: int, w: int, min_sizes: Sequence[int], max_size: int, flip: bool = True) -> List[Dict]:
    """detectron2 DatasetMapperTTA's list: per size the full frame at its ResizeShortestEdge target and, with `flip`, its mirrored
    twin right behind it."""
    views = []
    for s in min_sizes:
        size = resize_shortest_edge_shape(h, w, int(s), int(max_size))
        views.append(make_view((0, 0, w, h), size, False))
        if flip:
            views.append(make_view((0, 0, w, h), size, True))
    return views


def _tile_starts(extent: int, tile: int, overlap: float) -> List[int]:
    """Origins of `tile`-long windows over [0, extent) at a stride of tile * (1 - overlap); the last window is shifted inwards so that
    it ends at `extent`: every window is full and every position is covered."""
    if tile >= extent:
        return [0]
    step = max(1, int(math.floor(tile * (1.0 - overlap) + 1e-9)))
    n = int(math.ceil((extent - tile) / step)) + 1
    starts = []
    for i in range(n):
        s = min(i * step, extent - tile)
        if not starts or s != starts[-1]:
            starts.append(s)
    return starts


def tile_views(h: int, w: int, tile_hw: Sequence[int], overlap: float, size: Optional[int], max_size: int, full_frame: bool = True) -> List[Dict]:
    """A regular grid of tile_hw crops (clipped to the source) with fractional `overlap`, row by row; each tile is resized by the
    shortest-edge rule to (`size`, `max_size`) -- size None: kept at its own resolution.  With `full_frame` the whole source, resized by
    the same rule (size None: to the tile's shorter edge), comes first: it sees the objects that no tile holds whole."""
    if not 0.0 <= float(overlap) < 1.0:
        raise ValueError(f"tile overlap {overlap} must be in [0, 1)")
    th, tw = min(int(tile_hw[0]), h), min(int(tile_hw[1]), w)
    if th <= 0 or tw <= 0:
        raise ValueError(f"tile size {tuple(tile_hw)} must be positive")
    views = []
    if full_frame:
        views.append(make_view((0, 0, w, h), resize_shortest_edge_shape(h, w, int(size) if size is not None else min(th, tw), int(max_size))))
    tsize = resize_shortest_edge_shape(th, tw, int(size), int(max_size)) if size is not None else (th, tw)
    for y0 in _tile_starts(h, th, float(overlap)):
        for x0 in _tile_starts(w, tw, float(overlap)):
            views.append(make_view((x0, y0, tw, th), tsize))
    return views


def plan_view_steps(views: Sequence[Dict], max_batch: int = DEFAULT_MAX_BATCH, divisibility: int = 32) -> List[List[int]]:
    """Views -> steps (lists of view indices, ascending) of at most `max_batch` views.  The views of a step share the padded size their
    resize targets give (the batch is padded to the largest target, rounded up to `divisibility`), so a 400-pixel view is never padded
    to a 1200-pixel batch.  Groups come in the order their first view appears; the same list gives the same steps."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    d = max(1, int(divisibility))
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, v in enumerate(views):
        nh, nw = v["size"]
        groups.setdefault(((int(nh) + d - 1) // d * d, (int(nw) + d - 1) // d * d), []).append(i)
    steps = []
    for idx in groups.values():  # (insertion order)
        for k in range(0, len(idx), max_batch):
            steps.append(idx[k:k + max_batch])
    return steps


def view_out_size(view: Dict) -> Tuple[int, int]:
    """(height, width) the per-view decode scales its boxes to: the crop's own pixels."""
    return int(view["crop"][3]), int(view["crop"][2])


def merge_route(views_per_source: Sequence[int], max_in: int, topk: Optional[int]) -> str:
    """Which merge a view table takes: "block" -- Engine.merge_views, one block per source with its pool on chip -- when every source's
    views hold at most MERGE_POOL_CAP rows together (views x max_in) and rule 5's K is the config's (topk None); "large" --
    Engine.merge_views_large -- otherwise."""
    if topk is None and all(int(n) * int(max_in) <= MERGE_POOL_CAP for n in views_per_source):
        return "block"
    return "large"


DEFAULT_STITCH_THR = 0.5    # share of the smaller box that a cut fragment and its keeper must have in common
DEFAULT_STITCH_BORDER = 2.0  # pixels from an inner crop border within which a box counts as cut


def stitch_params(stitch) -> Optional[Tuple[float, float]]:
    """An input's "stitch" value -> (stitch_thr, border_px), None when stitching is off: True takes the defaults, a dict may carry "thr"
    and "border".  A threshold outside (0, 1], a negative border or an unknown key raises ValueError by name."""
    if stitch is None or stitch is False:
        return None
    if stitch is True:
        return DEFAULT_STITCH_THR, DEFAULT_STITCH_BORDER
    if not isinstance(stitch, dict) or set(stitch) - {"thr", "border"}:
        raise ValueError(f"\"stitch\" must be True or a dict with \"thr\" and / or \"border\", got {stitch!r}")
    thr, border = float(stitch.get("thr", DEFAULT_STITCH_THR)), float(stitch.get("border", DEFAULT_STITCH_BORDER))
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"\"stitch\": thr {thr} is outside (0, 1]")
    if not border >= 0.0:
        raise ValueError(f"\"stitch\": border {border} must be at least 0")
    return thr, border


def view_merge_route(views_per_source: Sequence[int], max_in: int, topk: Optional[int], stitch: Optional[Tuple[float, float]]) -> str:
    """merge_route with stitching: "stitch" -- Engine.stitch_views -- whenever the call asks for it (stitch_params gave a pair), whatever
    its size; otherwise merge_route's answer, unchanged."""
    if stitch is not None:
        return "stitch"
    return merge_route(views_per_source, max_in, topk)


def cut_flags(view: Dict, source_hw: Sequence[int], boxes_src, border_px: float):
    """Rule 0 of sylph_stitch_views in float32 on the host: boxes_src (N, 4) in SOURCE pixels (after the view's flip and offset) -> (N,)
    bool, True where a border of the view's crop that lies inside the (height, width) source cuts the box: the box comes within
    border_px of it.  A crop border that is the source's own never cuts."""
    import numpy as np
    f = np.float32
    b = np.asarray(boxes_src, dtype=f).reshape(-1, 4)
    x0, y0, cw, ch = (f(t) for t in view["crop"])
    sh, sw, bp = f(source_hw[0]), f(source_hw[1]), f(border_px)
    left, top, right, bottom = x0, y0, f(x0 + cw), f(y0 + ch)
    cut = np.zeros(len(b), dtype=bool)
    if left > 0:
        cut |= b[:, 0] <= f(left + bp)
    if right < sw:
        cut |= b[:, 2] >= f(right - bp)
    if top > 0:
        cut |= b[:, 1] <= f(top + bp)
    if bottom < sh:
        cut |= b[:, 3] >= f(bottom - bp)
    return cut
