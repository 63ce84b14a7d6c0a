"""Shot bank: the per-shot rows of a pool of annotated support instances (Engine.codegen_shots), kept on the device, and the draws of
K shots per class that Engine.combine_shots turns into class codes without a network pass.  The support-side counterpart of the
query records: a seed or shot sweep over one annotated pool pays the backbone and the code-generator tower once per image.

A bank holds no pyramid: a new box on a banked image needs that image again.  Its rows are valid only under the weights, dtype and
generator config that made them; the config part is kept as the bank's key and checked against the engine, the weights are the
caller's responsibility."""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

KEY_FIELDS = ("generator", "code_ksize", "dtype", "row_floats")


def _ints(v) -> List[int]:
    return [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]


class ShotBank:
    """rows (n, row_floats) fp32 on `device` + per row class_id, image_id, ann_id (host lists) + the key it was made under
    (KEY_FIELDS: generator type, code kernel size, dtype, row width; Engine.shot_key())."""

    def __init__(self, key: Dict[str, Any], device=None):
        missing = [f for f in KEY_FIELDS if f not in key]
        if missing:
            raise ValueError(f"shot bank key lacks {missing}")
        self.key = {f: key[f] for f in KEY_FIELDS}
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.rows = torch.empty(0, int(self.key["row_floats"]), dtype=torch.float32, device=self.device)
        self.class_ids: List[int] = []
        self.image_ids: List[int] = []
        self.ann_ids: List[int] = []
        self._parts: List[torch.Tensor] = []  # appended chunks not yet concatenated into rows
        self.stamp = 0  # Engine.codegen_stamp() when the rows were made: 0 = the checkpoint's generator (build_shot_bank sets it)

    def __len__(self) -> int:
        return len(self.class_ids)

    @property
    def row_floats(self) -> int:
        return int(self.key["row_floats"])

    @property
    def nbytes(self) -> int:
        """bytes of the row tensor"""
        return len(self) * self.row_floats * 4

    def append(self, rows: torch.Tensor, class_ids: Sequence[int], image_ids: Sequence[int], ann_ids: Sequence[int]):
        """Add the rows of one codegen_shots call with what identifies each: its class, its image and its annotation index."""
        if rows.dim() != 2 or rows.shape[1] != self.row_floats or rows.dtype != torch.float32:
            raise ValueError(f"shot bank: rows of shape {tuple(rows.shape)} {rows.dtype}, the bank's rows are {self.row_floats} fp32 floats wide")
        cls, img, ann = _ints(class_ids), _ints(image_ids), _ints(ann_ids)
        if not (len(cls) == len(img) == len(ann) == rows.shape[0]):
            raise ValueError(f"shot bank: {rows.shape[0]} rows with {len(cls)} class ids, {len(img)} image ids, {len(ann)} annotation ids")
        self._parts.append(rows.detach().to(self.device).clone())
        self.class_ids += cls
        self.image_ids += img
        self.ann_ids += ann
        return self

    def tensor(self) -> torch.Tensor:
        """the bank's rows as ONE contiguous device tensor (appended chunks are concatenated on first use)"""
        if self._parts:
            self.rows = torch.cat([self.rows] + self._parts).contiguous()
            self._parts = []
        return self.rows

    def classes(self) -> List[int]:
        return sorted(set(self.class_ids))

    def rows_of(self, class_id: int) -> List[int]:
        """row numbers of a class's instances, in bank order"""
        c = int(class_id)
        return [r for r, k in enumerate(self.class_ids) if k == c]

    def draw(self, shots: int, seed: int, classes: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int], List[int]]:
        """K shots per class -> (idx, seg_len, class_ids): per class in ascending class id (all banked classes, or `classes`), a choice
        of `shots` of its rows without replacement from numpy.random.RandomState(seed) -- one generator for the whole draw, consumed
        in class order; a class with no more than `shots` instances gives all of them, in bank order, and draws nothing."""
        shots = int(shots)
        if shots < 1:
            raise ValueError(f"shots must be at least 1, got {shots}")
        rng = np.random.RandomState(int(seed))
        want = self.classes() if classes is None else sorted({int(c) for c in classes})
        idx, seg_len, cids = [], [], []
        for c in want:
            pool = self.rows_of(c)
            if not pool:
                raise ValueError(f"shot bank: class {c} has no banked instance")
            pick = pool if len(pool) <= shots else [pool[i] for i in rng.choice(len(pool), shots, replace=False).tolist()]
            idx += pick
            seg_len.append(len(pick))
            cids.append(c)
        return idx, seg_len, cids

    def check_key(self, engine) -> None:
        """refuse, naming the field, a bank made under another generator config than `engine`'s"""
        theirs = engine.shot_key()
        for f in KEY_FIELDS:
            if self.key[f] != theirs[f]:
                raise ValueError(f"shot bank: made with {f} = {self.key[f]!r}, the engine has {f} = {theirs[f]!r}; its rows are valid only "
                                 "under the weights, dtype and generator config that made them")

    def check_stamp(self, engine) -> None:
        """refuse a bank whose rows were made by another generator than the one `engine` runs now (Engine.set_code_generator)"""
        now = int(engine.codegen_stamp())
        if int(self.stamp) != now:
            raise ValueError(f"shot bank: its rows were made under generator stamp {int(self.stamp)}, the engine now runs stamp {now} "
                             "(set_code_generator installed another generator since): build the bank again under the current generator, or "
                             "restore the one it was made under (set_code_generator(None) for stamp 0)")

    def save(self, path: str) -> None:
        torch.save({"key": dict(self.key), **({"stamp": int(self.stamp)} if int(self.stamp) else {}),  # (a bank of the checkpoint's generator saves what it always saved)
                    "rows": self.tensor().cpu(), "class_ids": list(self.class_ids), "image_ids": list(self.image_ids),
                    "ann_ids": list(self.ann_ids)}, path)

    @classmethod
    def load(cls, path: str, engine=None, device=None) -> "ShotBank":
        """The saved bank, on `device` (default: the engine's, else the CPU).  With an engine the key is checked (check_key)."""
        d = torch.load(path, map_location="cpu")
        bank = cls(d["key"], device=device if device is not None else (engine.device if engine is not None else None))
        bank.stamp = int(d.get("stamp", 0))
        if engine is not None:
            bank.check_key(engine)
        if len(d["class_ids"]):
            bank.append(d["rows"], d["class_ids"], d["image_ids"], d["ann_ids"])
        return bank
