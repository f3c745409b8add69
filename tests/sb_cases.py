"""The batch-fastest kernel's variant space as a checked object: the rows of `SMM_BUILT` (smmregrid_amd/csrc/smm_built.hpp)
read from the header and mapped to the Python call that reaches each; the instantiations of `sb_tile_body`
(smm_kernels.hpp) that `launch_sb_any` / `with_sb_tile_rows` (smm_launch.hpp) can pick; the tile order restated; and
the synthetic operators, fields and float64 references the GPU test walks.  Plain numpy, no GPU.

A cell is `Cell(row, skipna, td, u, fill, ysb, kind)`:

  row     a row of SMM_BUILT: `Row(x, dd, y)` -- field kind, decode dtype of a packed field (else None), result kind
  skipna  SMM_APPLY_SKIPNA
  td      destination rows per tile: 16 (8-byte Y), 32 (4-byte Y), 64 or 16 (2-byte Y, sb_packed_y_rows)
  u       loads per batch: 8, or 4 (sb_loads)
  fill    False = SMM_APPLY_NO_FILL (refused with skipna)
  ysb     the result kept batch-fastest (SMM_APPLY_SB_Y_SB)
  kind    "single" (smm_apply_sb_kernel) or "group" (smm_group_apply_sb_kernel)

The operators.  The destination grid is N_FULL = 11 whole tiles followed by a tail of r rows, n_dst = 11 td + r: one
whole tile for each kind of tile the link walk tells apart (TILE_KINDS: no link; 1, U - 1, U, U + 1, 2 U and 2 U + 1
links for U = 4 and U = 8; a row of more than 4 U links among short ones).  Two whole tiles and the tail -- three
tiles -- cannot hold them, and every cell is meant to meet every kind in one launch.  The tail rule is kept: r = 3 for
every cell, r in {1, 2, td - 1, td} swept by the tail test.

The reference of a case is the float64 result of the CPU oracles (`oracle.apply_c`, `oracle.apply_levels`,
`tests.helpers.skipna_ref`) on the values the kernel's X stands for, narrowed by the row's own rule (`narrow`).  It is
computed for B_MAX batch entries once; a launch of B entries is compared with its first B rows (batch entries are
independent), so the fields are made once and left unchanged."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import oracle
from smmregrid_amd import CFDecode, CFEncode, _lib, bfloat16
from tests import half_cases as hc
from tests.helpers import skipna_ref

Row = namedtuple("Row", "x dd y")
Cell = namedtuple("Cell", "row skipna td u fill ysb kind")

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smmregrid_amd", "csrc",
                      "smm_built.hpp")
SEED = 20261019
KINDS = ("single", "group")
US = (8, 4)
N_SRC = 97                        # odd: 2-byte rows start off 4-byte boundaries
BATCHES = (1, 2, 3, 127, 128, 129, 257)
B_MAX = max(BATCHES)
TAIL_BATCHES = (1, 3, 129)
R_CELLS = 3                       # the tail every cell gets
LONG = 37                         # one row alone longer than 4 U = 32 links
TILE_KINDS = ("empty", 1, 3, 4, 5, 7, 8, 9, 16, 17, "long")
N_FULL = len(TILE_KINDS)
LOW = 30                          # batch entry 0 is invalid on source cells [0, LOW); tiles of 3 and 4 links draw from them
BIG_COL = 40                      # batch entry 0 holds 1e20 there where the type can
LEVEL_INDEX = (2, 0, 1, 2)
MASKED_LEVELS = (1, 0, 1)         # group member 1 runs with L.imask == nullptr
# (masked, remap_area_min, operator keeps its dst_frac).  remap_area_min > 0 without dst_frac is refused by the
# library, so the epilogue without dst_frac runs at remap_area_min = 0 (single kernel only)
EPILOGUES = ((False, 0.0, True), (True, 0.37, True), (True, 0.0, False))
GROUP_EPILOGUES = EPILOGUES[:2]
SENTINEL = 0xA5                   # byte the GPU test pre-fills Y with

# (X dtype code, decode dtype, XT) -> (field kind, decode kind); (Y dtype code, YT) -> result kind
_X_OF = {("SMM_F64", "kAnyDecode", "double"): ("f64", None), ("SMM_F32", "kAnyDecode", "float"): ("f32", None),
         ("SMM_I16", "SMM_F32", "XI16F"): ("i16", "f32"), ("SMM_I16", "SMM_F64", "XI16D"): ("i16", "f64"),
         ("SMM_U16", "SMM_F32", "XU16F"): ("u16", "f32"), ("SMM_U16", "SMM_F64", "XU16D"): ("u16", "f64"),
         ("SMM_F16", "kAnyDecode", "XF16"): ("f16", None), ("SMM_BF16", "kAnyDecode", "XBF16"): ("bf16", None)}
_Y_OF = {("SMM_F64", "double"): "f64", ("SMM_F32", "float"): "f32", ("SMM_I16", "YI16"): "i16",
         ("SMM_U16", "YU16"): "u16", ("SMM_F16", "YF16"): "f16", ("SMM_BF16", "YBF16"): "bf16"}
NP_OF = {"f64": np.dtype(np.float64), "f32": np.dtype(np.float32), "i16": np.dtype(np.int16),
         "u16": np.dtype(np.uint16), "f16": np.dtype(np.float16), "bf16": bfloat16}
Y_SIZE = {"f64": 8, "f32": 4, "i16": 2, "u16": 2, "f16": 2, "bf16": 2}
TDS_OF_SIZE = {8: (16,), 4: (32,), 2: (64, 16)}          # with_sb_tile_rows / sb_tile_rows
_FILL = {"i16": -32768, "u16": 65535}


# ------------------------------------------------------------------ the rows

def parse_built(text):
    """The rows of SMM_BUILT in header order.  A line of the macro that is no M(...) row, or a row the tables above
    cannot map, is a ValueError."""
    lines = text.splitlines()
    start = [i for i, ln in enumerate(lines) if re.match(r"\s*#define\s+SMM_BUILT\(M\)", ln)]
    if len(start) != 1:
        raise ValueError("smm_built.hpp: expected one '#define SMM_BUILT(M)'")
    rows, i = [], start[0]
    while lines[i].rstrip().endswith("\\"):
        i += 1
        m = re.fullmatch(r"\s*M\((\w+),\s*(\w+),\s*(\w+),\s*(\w+),\s*(\w+),\s*([01])\)\s*\\?\s*", lines[i])
        if not m:
            raise ValueError(f"smm_built.hpp line {i + 1}: not an M(x_dtype, decode_dtype, XT, y_dtype, YT, TILE) row")
        xd, dd, xt, yd, yt, _ = m.groups()
        if (xd, dd, xt) not in _X_OF or (yd, yt) not in _Y_OF:
            raise ValueError(f"smm_built.hpp line {i + 1}: no Python call is known for {m.group(0).strip()}")
        rows.append(Row(*_X_OF[(xd, dd, xt)], _Y_OF[(yd, yt)]))
    if len(set(rows)) != len(rows):
        raise ValueError("smm_built.hpp: a row of SMM_BUILT is listed twice")
    return rows


def built_rows():
    with open(HEADER) as f:
        return parse_built(f.read())


ROWS = built_rows()


def row_id(row):
    return f"{row.x}{'>' + row.dd if row.dd else ''}-{row.y}"


def decoder(row, fill=True):
    """The CFDecode of a packed field (None for any other): NO_FILL is refused with fill values, so it takes none."""
    if row.x not in _FILL:
        return None
    return CFDecode(0.125, 20.0 if row.x == "i16" else -4000.0, (_FILL[row.x],) if fill else (), NP_OF[row.dd])


def encoder(row):
    """The CFEncode of a packed result (None for any other).  A packed field's values are a hundred times a float
    field's: a coarser scale keeps most results inside the raw range."""
    if row.y not in _FILL:
        return None
    scale = 8.0 if row.x in _FILL else 0.25
    return CFEncode(scale, -0.125 if row.y == "i16" else -(32768.0 * scale) - 0.125, _FILL[row.y], NP_OF[row.y])


def call_of(row, fill=True):
    """What `apply_sb` takes to reach the row: the field's dtype and the keywords cf, cf_out, out_dtype."""
    cf_out = encoder(row)
    return dict(x_dtype=NP_OF[row.x], cf=decoder(row, fill), cf_out=cf_out,
                out_dtype=np.dtype(np.float64) if cf_out is not None else NP_OF[row.y])


# ------------------------------------------------------------------ the cells

def cells(rows=None):
    """Every instantiation `launch_sb_any` can pick: per row, per kernel (2), per tile height of the row's Y element
    size (1, or 2 for a 2-byte Y), per U (2), per YSB (2): plain with FILL, plain without, skipna (3).  With the
    header's n1 rows of an 8- or 4-byte Y and n2 rows of a 2-byte Y that is 24 (n1 + 2 n2) cells."""
    out = []
    for row in ROWS if rows is None else rows:
        for skipna, fill in ((False, True), (False, False), (True, True)):
            for td in TDS_OF_SIZE[Y_SIZE[row.y]]:
                for u in US:
                    for ysb in (False, True):
                        for kind in KINDS:
                            out.append(Cell(row, skipna, td, u, fill, ysb, kind))
    return out


def expected_cell_count(rows=None):
    rows = ROWS if rows is None else rows
    n2 = sum(Y_SIZE[r.y] == 2 for r in rows)
    return 24 * ((len(rows) - n2) + 2 * n2)


def launch_of(cell):
    """(tuning knobs, apply flags, keep_batch_fastest) that make the library pick the cell."""
    knobs = {"sb_loads": cell.u, "sb_packed_y_rows": 16 if (Y_SIZE[cell.row.y] == 2 and cell.td == 16) else 0}
    return knobs, (0 if cell.fill else _lib.APPLY_NO_FILL), cell.ysb


# one GPU test per (row, skipna, kind); it walks these cells
TESTS = [(row, skipna, kind) for row in ROWS for skipna in (False, True) for kind in KINDS]


def cells_of_test(row, skipna, kind):
    return [c for c in cells([row]) if c.skipna == skipna and c.kind == kind]


def epilogues_of(kind):
    return EPILOGUES if kind == "single" else GROUP_EPILOGUES


def launches():
    """Kernel launches of the per-cell tests: every cell at every batch under its epilogues, a group once per
    transpose setting unless the result is kept batch-fastest (the setting then plays no part)."""
    n = 0
    for c in cells():
        per = len(epilogues_of(c.kind)) * (2 if c.kind == "group" and not c.ysb else 1)
        n += per * len(BATCHES)
    return n


# ------------------------------------------------------------------ the tile order

def xcd_remap_block(bid, run, n_blocks):
    """`xcd_remap_block` of smm_kernels.hpp."""
    if run > 0:
        rnd = 8 * run
        if bid < (n_blocks // rnd) * rnd:
            xcd, slot = bid & 7, bid >> 3
            bid = (slot // run) * rnd + xcd * run + slot % run
    return bid


def tile_of(bid, n_dtiles, n_btiles, strip, run):
    """Workgroup -> (destination tile, batch tile): the remap, then the `b_fastest` strip arithmetic of sb_tile_body.
    strip = args.b_fastest (0: destination tile fastest over the whole grid), run = args.xcd_remap."""
    bid = xcd_remap_block(bid, run, n_dtiles * n_btiles)
    if strip > 0:
        per = n_btiles * strip
        sd = bid // per
        rem = bid - sd * per
        here = min(n_dtiles - sd * strip, strip)
        bt = rem // here
        return sd * strip + (rem - bt * here), bt
    bt = bid // n_dtiles
    return bid - bt * n_dtiles, bt


def order_args(sb_strip=0, xcd_run=0):
    """(b_fastest, xcd_remap) `launch_sb_any` derives from the two knobs."""
    return (0 if sb_strip < 0 else (sb_strip or 2)), (0 if xcd_run < 0 else (xcd_run or 32))


def remapped_blocks(n_blocks, run):
    return (n_blocks // (8 * run)) * 8 * run if run > 0 else 0


def choose_order(n_dtiles, n_btiles):
    """(sb_strip, xcd_run), neither the default: the remapped part lies strictly inside the grid (both branches of
    the remap are taken) and the last strip is short."""
    n = n_dtiles * n_btiles
    for run in range(6, 0, -1):
        for strip in range(5, 0, -1):
            if 0 < remapped_blocks(n, run) < n and n_dtiles % strip and strip < n_dtiles and strip != 2 and run != 32:
                return strip, run
    raise ValueError(f"no (strip, run) for a grid of {n_dtiles} x {n_btiles} tiles")


def n_dst_of(td, r):
    return N_FULL * td + r


def order_grid(td):
    """(n_dtiles, n_btiles) of the tile-order test: the largest n_dst of the height, B = 257."""
    return -(-n_dst_of(td, td) // td), -(-B_MAX // 128)


# ------------------------------------------------------------------ the operators

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def links(td, r, member=0):
    """SCRIP links (1-based, shuffled, with duplicate (dst, src) pairs) of one operator on the grid of (td, r):
    (src, dst, w, tile kinds in grid order).  The whole tiles are a permutation of TILE_KINDS; the tile of 5 links
    starts with three empty rows, the tile of 9 ends with three; the tail's rows hold 0 .. 3 links."""
    rng = np.random.default_rng([SEED, td, r, member])
    n_dst = n_dst_of(td, r)
    kinds = [TILE_KINDS[k] for k in rng.permutation(N_FULL)]
    lens = np.zeros(n_dst, np.int64)
    low = np.zeros(n_dst, bool)
    for t, kind in enumerate(kinds):
        d0 = t * td
        if kind == "empty":
            continue
        if kind == "long":
            lens[d0:d0 + td] = rng.integers(0, 7, size=td)
            lens[d0 + int(rng.integers(td))] = LONG
            continue
        lo, hi = (3, td) if kind == 5 else ((0, td - 3) if kind == 9 else (0, td))
        np.add.at(lens, d0 + rng.integers(lo, hi, size=kind), 1)
        low[d0:d0 + td] = kind in (3, 4)
    lens[N_FULL * td:] = rng.integers(0, 4, size=r)
    lens[-1] = max(lens[-1], 2)                               # the tail is never without links
    src, dst, w = [], [], []
    for d in np.nonzero(lens)[0]:
        cols = rng.choice(LOW if low[d] else N_SRC, size=int(lens[d]), replace=False)
        if lens[d] == LONG and BIG_COL not in cols:
            cols[0] = BIG_COL                                 # the cell that holds 1e20 is linked
        ww = rng.uniform(-0.5, 1.5, size=cols.size)
        ww[rng.random(cols.size) < 0.05] = 0.0                # exact zeros: links like any other
        if low[d]:
            ww[ww == 0.0] = 0.75                              # rows that batch entry 0 leaves without a valid link
        two = rng.random(cols.size) < 0.1                     # a link written twice: the pair sums to its weight
        src += [cols, cols[two]]
        dst += [np.full(cols.size + int(two.sum()), d)]
        w += [np.where(two, 0.25 * ww, ww), 0.75 * ww[two]]
    src, dst, w = np.concatenate(src), np.concatenate(dst), np.concatenate(w)
    perm = rng.permutation(src.size)
    src, dst, w = _frozen((src[perm] + 1).astype(np.int32), (dst[perm] + 1).astype(np.int32), w[perm])
    return src, dst, w, tuple(kinds)


@functools.lru_cache(maxsize=None)
def operator(td, r, member=0):
    """dict(n_dst, src, dst, w, csr, imask, frac, kinds): the oracle's CSR of the links, about 10 % of dst_imask zero, dst_frac in
    [0.2, 1): about a fifth below the 0.37 of the epilogues."""
    src, dst, w, kinds = links(td, r, member)
    n_dst = n_dst_of(td, r)
    rng = np.random.default_rng([SEED, td, r, member, 1])
    imask, frac = _frozen((rng.random(n_dst) > 0.1).astype(np.int32), 0.2 + 0.8 * rng.random(n_dst))
    csr = _frozen(*oracle.coo_to_csr(N_SRC, n_dst, src, dst, w))
    return dict(n_dst=n_dst, src=src, dst=dst, w=w, csr=csr, imask=imask, frac=frac, kinds=kinds)


def tile_links(op, td):
    """Links per tile of the operator's CSR."""
    rowptr = op["csr"][0]
    edges = np.minimum(np.arange(0, op["n_dst"] + td, td), op["n_dst"])
    return np.diff(rowptr[edges])


def rows_without_valid_link(op):
    """Destination rows whose links all lie on the cells batch entry 0 holds invalid, none of weight zero."""
    rowptr, col, val = op["csr"]
    return [d for d in range(op["n_dst"]) if rowptr[d + 1] > rowptr[d]
            and (col[rowptr[d]:rowptr[d + 1]] < LOW).all() and (val[rowptr[d]:rowptr[d + 1]] != 0.0).all()]


# ------------------------------------------------------------------ the fields

def _marks(rng, shape):
    u = rng.random(shape)
    return u < 0.03, (u >= 0.03) & (u < 0.035), rng.random(shape) < 0.5       # NaN, inf, its sign


@functools.lru_cache(maxsize=None)
def field(x, dd=None, fill=True, level=0):
    """(what the kernel reads, the float32 / float64 values it stands for), both (B_MAX, N_SRC): about 3 % NaN and
    0.5 % +-inf (a packed field: 3.5 % fill values, none under NO_FILL), batch entry 0 invalid on [0, LOW), 1e20 at
    [0, BIG_COL] where the type holds it."""
    rng = np.random.default_rng([SEED, 7, sorted(NP_OF).index(x), level])
    shape = (B_MAX, N_SRC)
    if x in _FILL:
        info = np.iinfo(NP_OF[x])
        q = rng.integers(info.min, info.max + 1, size=shape).astype(NP_OF[x])
        q[q == _FILL[x]] = 77
        nan, inf, _ = _marks(rng, shape)
        if fill:
            q[nan | inf] = _FILL[x]
            q[0, :LOW] = _FILL[x]
        return _frozen(q, decoder(Row(x, dd, "f64"), fill).decode(q))
    v = 40.0 * rng.standard_normal(shape)
    nan, inf, neg = _marks(rng, shape)
    v[nan] = np.nan
    v[inf] = np.where(neg[inf], -np.inf, np.inf)
    v[0, :LOW] = np.nan
    if x != "f16":
        v[0, BIG_COL] = 1e20
    if x in ("f16", "bf16"):
        with np.errstate(over="ignore"):
            bits = hc.round_bits(v, x)
        return _frozen(bits.view(NP_OF[x]), hc.widen(bits, x))
    v = v.astype(NP_OF[x])
    return _frozen(v, v)


# ------------------------------------------------------------------ the references

def _apply64(op, xv, skipna, fill, masked, area_min, has_frac):
    frac = op["frac"] if has_frac else None
    if skipna:
        return skipna_ref(op["csr"], xv, masked, op["imask"], frac, area_min)
    return oracle.apply_c(op["csr"], xv, masked, op["imask"], frac, area_min, fill=fill)


@functools.lru_cache(maxsize=48)
def reference64(x, dd, skipna, fill, kind, td, r, epilogue):
    """float64 result for B_MAX batch entries: (B_MAX, D) of the single operator, (L, B_MAX, D) of the group."""
    masked, area_min, has_frac = epilogue
    ffill = fill if x in _FILL else True          # a float field is the same under NO_FILL
    if kind == "single":
        return _frozen(_apply64(operator(td, r), field(x, dd, ffill)[1], skipna, fill, masked, area_min,
                                has_frac))[0]
    ops = [operator(td, r, m) for m in range(len(MASKED_LEVELS))]
    xs = [field(x, dd, ffill, level)[1] for level in range(len(LEVEL_INDEX))]
    if not skipna and fill:
        ml = np.array(MASKED_LEVELS, bool) & masked
        y = oracle.apply_levels([o["csr"] for o in ops], np.stack(xs, axis=1), 1, np.array(LEVEL_INDEX), ml,
                                np.stack([o["imask"] for o in ops]), np.stack([o["frac"] for o in ops]), area_min,
                                transpose=False)
    else:
        y = np.stack([_apply64(ops[w], xs[l], skipna, fill, masked and bool(MASKED_LEVELS[w]), area_min, has_frac)
                      for l, w in enumerate(LEVEL_INDEX)])
    return _frozen(y)[0]


def narrow(y64, row):
    """The float64 result as Y must hold it: float64 / float32 as floats, a 2-byte Y as its raw uint16 / int16 bits."""
    if row.y == "f64":
        return y64
    if row.y == "f32":
        with np.errstate(over="ignore"):
            return y64.astype(np.float32)
    if row.y in _FILL:
        return encoder(row).encode(y64)
    return hc.round_bits(y64, row.y)


@functools.lru_cache(maxsize=48)
def reference(row, skipna, fill, kind, td, r, epilogue):
    return _frozen(narrow(reference64(row.x, row.dd, skipna, fill, kind, td, r, epilogue), row))[0]


def missing(ref, row):
    """Cells of a narrowed reference that hold NaN or the fill value."""
    if row.y in _FILL:
        return ref == _FILL[row.y]
    if row.y in ("f16", "bf16"):
        return ref == hc.KINDS[row.y][2]
    return np.isnan(ref)


def finite(ref, row):
    if row.y in _FILL:
        return ref != _FILL[row.y]
    if row.y in ("f16", "bf16"):
        return np.isfinite(hc.widen(ref, row.y))
    return np.isfinite(ref)


# ------------------------------------------------------------------ the rotations of the tile-order and tail tests

SIZE_TD = ((8, 16), (4, 32), (2, 64), (2, 16))       # (Y element size, tile height): every pair that is built


def rows_of_size(size):
    return [r for r in ROWS if Y_SIZE[r.y] == size]


def rotated(size, i):
    """(row, skipna, u) number i of a rotation over the rows of a Y element size."""
    rows = rows_of_size(size)
    return rows[i % len(rows)], bool((i // 2) % 2), US[i % 2]
