"""The rule of categorical regridding -- largest area fraction, the "mode" -- stated once in numpy.

A field of class codes (land cover, soil and vegetation type, basin and land-sea masks, precipitation type) must not be
averaged: classes 3 and 7 do not make class 5.  `ModeRule.apply` says what `SparseOperator.apply_mode` (smm_apply_mode)
computes instead; it is the definition the device kernel is tested against bit for bit, as `CFEncode.encode` and
`GradientRule.gradients` are for theirs.  Host only: numpy, no device.

For destination row d, batch row b and the links k of the canonical CSR in ascending source order, w_k the weight of
column 0:

* Missing values.  A float field's ``x[b, col_k]`` is missing when it is not finite; an integer field's when it equals
  one of the rule's `fill` values (at most two), compared on the raw integer.  A missing link takes part in no class.
* Classes.  Two links are of one class when their values compare equal with ``==`` (``-0.0`` and ``+0.0`` are one
  class); a class is represented by the value of its first link.  ``share(c)`` is the sum of w_k over the links of class
  c, in float64, from ``+0.0``, in ascending link order, one add per link -- exactly the bits of the plain apply on the
  float64 indicator field ``x == c``.
* Row sums.  ``tot`` is the sum of w_k over all links of the row, ``val`` the same over the links that are not missing,
  both in that order from ``+0.0``.
* Winner.  The class of the largest share, which must be ``> 0.0``; bit-equal shares go to the class whose first link
  comes first.
* Dead rows.  A row is dead when it is masked, when no class has a share > 0 (no links, all missing, all weights <= 0),
  or when ``remap_area_min > 0`` and ``frac_d * (val / tot) < remap_area_min`` (``frac_d = dst_frac[d]``).
* Result.  ``y[b, d]`` has the field's own dtype and holds the winner's representative value bit for bit; a dead row
  holds NaN (floats) or `fill_out` (integers).  ``share[b, d]`` holds the winner's share as summed above, undivided; a
  dead row ``+0.0``.

This is CDO's `remaplaf` as recalled; it is not pinned against a `cdo` run.  Weights of ``method="laf"`` are the static
one-cell approximation of it (one link per target cell, to the source cell of largest overlap, whatever the values);
conservative weights with this rule give the area-weighted mode.
"""
import numpy as np

BUILT_DTYPES = (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int16), np.dtype(np.uint16))
# host fields widened exactly to int16 on the way in and narrowed back on the way out (apply_mode_host)
WIDENED_DTYPES = (np.dtype(np.int8), np.dtype(np.uint8))


def built_words():
    return "float32, float64, int16, uint16" + " (and int8 / uint8 host fields, widened to int16)"


class ModeRule:
    """The missing values of a class field and what a dead row stores.

    fill: for an integer field, the raw values that are missing (none, one or two); a float field takes none -- its
    missing value is whatever is not finite.  fill_out: what a dead row of an integer field stores (default: the first
    of `fill`); a float field's dead rows are NaN."""

    def __init__(self, fill=(), fill_out=None):
        self.fill = tuple(int(v) for v in np.atleast_1d(np.asarray(fill, dtype=np.int64)).ravel()) if np.size(fill) else ()
        if len(self.fill) > 2:
            raise ValueError(f"a class field has at most two fill values, got {len(self.fill)}")
        self.fill_out = None if fill_out is None else int(fill_out)

    @classmethod
    def from_attrs(cls, attrs, dtype):
        """The rule of an integer variable's attributes: `fill` its distinct `_FillValue` / `missing_value` in that
        order, `fill_out` the first of them.  (rule, found): without either attribute the dtype's minimum (signed) or
        maximum (unsigned) is used and found is False."""
        dtype = np.dtype(dtype)
        if dtype.kind == "f":
            return cls(), True
        fills = []
        for key in ("_FillValue", "missing_value"):
            if key in attrs:
                for v in np.atleast_1d(np.asarray(attrs[key])).ravel():
                    if int(v) not in fills:
                        fills.append(int(v))
        if fills:
            return cls(fills, fills[0]), True
        info = np.iinfo(dtype)
        edge = int(info.min if dtype.kind == "i" else info.max)
        return cls((edge,), edge), False

    def checked(self, dtype):
        """(fill, fill_out) for a field of `dtype`, or a ValueError / TypeError naming what does not fit."""
        dtype = np.dtype(dtype)
        if dtype.kind == "f":
            if self.fill or self.fill_out is not None:
                raise ValueError("a float class field takes no fill / fill_out: its missing value is whatever is not finite")
            return (), None
        if dtype.kind not in "iu":
            raise TypeError(f"a class field is {built_words()}, not {dtype}")
        info = np.iinfo(dtype)
        fill_out = self.fill_out if self.fill_out is not None else (self.fill[0] if self.fill else None)
        if fill_out is None:
            raise ValueError("an integer class field needs fill_out (or a fill value to take it from): what a dead row stores")
        for name, v in [("fill", v) for v in self.fill] + [("fill_out", fill_out)]:
            if not info.min <= v <= info.max:
                raise ValueError(f"{name}={v} is no value of {dtype}")
        return self.fill, fill_out

    def missing(self, x):
        """Which cells of x are missing."""
        x = np.asarray(x)
        if x.dtype.kind == "f":
            return ~np.isfinite(x)
        out = np.zeros(x.shape, dtype=bool)
        for v in self.fill:
            out |= x == v
        return out

    def apply(self, csr, x, masked=False, dst_imask=None, dst_frac=None, remap_area_min=0.0):
        """(y, share) of the (B, >= S) field x on the canonical CSR (rowptr, col, val) -- what `export_csr` returns."""
        rowptr, col, val = (np.asarray(a) for a in csr)
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError(f"x must be (B, S), got {x.shape}")
        fill, fill_out = self.checked(x.dtype)
        if masked and dst_imask is None:
            raise ValueError("masked apply requested but there is no dst_imask")
        if remap_area_min > 0.0 and dst_frac is None:
            raise ValueError("remap_area_min > 0 requested but there is no dst_frac")
        n_batch, n_dst = x.shape[0], rowptr.size - 1
        dead_value = np.nan if x.dtype.kind == "f" else fill_out
        y = np.full((n_batch, n_dst), dead_value, dtype=x.dtype)
        share_out = np.zeros((n_batch, n_dst), dtype=np.float64)
        for d in range(n_dst):
            lo, hi = int(rowptr[d]), int(rowptr[d + 1])
            n = hi - lo
            if n == 0 or (masked and dst_imask[d] == 0):
                continue
            w = np.asarray(val[lo:hi], dtype=np.float64)
            xv = x[:, col[lo:hi]]                      # (B, n)
            miss = self.missing(xv)
            tot = np.float64(0.0)
            vsum = np.zeros(n_batch)
            for k in range(n):
                tot = tot + w[k]
                vsum = np.where(miss[:, k], vsum, vsum + w[k])
            best_share = np.zeros(n_batch)
            best_k = np.full(n_batch, -1)
            for k in range(n):
                v = xv[:, k]
                cand = ~miss[:, k]
                if k:
                    cand &= ~(xv[:, :k] == v[:, None]).any(axis=1)
                if not cand.any():
                    continue
                share = np.zeros(n_batch)
                for j in range(k, n):
                    same = (xv[:, j] == v) if j > k else np.ones(n_batch, dtype=bool)
                    share = np.where(same, share + w[j], share)
                better = cand & (share > best_share)
                best_share = np.where(better, share, best_share)
                best_k = np.where(better, k, best_k)
            alive = best_k >= 0
            if remap_area_min > 0.0:
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    alive &= ~(np.float64(dst_frac[d]) * (vsum / tot) < remap_area_min)
            rows = np.flatnonzero(alive)
            y[rows, d] = xv[rows, best_k[rows]]
            share_out[rows, d] = best_share[rows]
        return y, share_out

    def __repr__(self):
        return f"ModeRule(fill={self.fill}, fill_out={self.fill_out})"
