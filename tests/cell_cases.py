"""The tile kernel's dispatch table as a checked object: which template instantiation of `smm_apply_tile2_kernel`
`launch_tile` (smmregrid_amd/csrc/smm_launch.hpp) picks, restated from observable facts; the set of cells it can
pick at all; synthetic operators that land in a requested cell; and the list of cases the GPU test walks.  Plain
numpy, no GPU.

A structural cell is `Cell(shape, maxk, np, r, staging, split, sub_shift)`:

  shape      destination rows per block of the tile plan: 256 (4 waves) or 64 / 32 / 16 / 8 (one wave)
  maxk       link registers per row: 4 / 8 / 16 (4 waves), 32 / 48 (one wave), 0 = links streamed from L2
  np         the kernel's NP: staging pieces per thread the instantiation is built for
  r          batch rows per barrier pair
  staging    "reg" or "dma" (LDS-DMA ring)
  split      rows split over lane groups (part-of-a-slice blocks)
  sub_shift  block = 1 / 2^sub_shift of a slice

NT, SKIPNA, XT and YT are the other template axes: `CASES` rotates them over the structural cells.

Two restatements live here and are kept apart on purpose.  `structural_cell` reads the cell off what
`launch_info` reports (the GPU test feeds it the library's answer); `model_launch_info` predicts what
`launch_info` will report from the links alone (planner and launcher restated), so that a case that would drift
out of its declared cell is caught on a machine without a GPU."""
import functools
from collections import namedtuple

import numpy as np

Cell = namedtuple("Cell", "shape maxk np r staging split sub_shift")
Case = namedtuple("Case", "id op xt yt knobs masked area_min skipna batch cell np_needed")

CHUNK = 4                                       # source elements per staged chunk
SHAPES = (256, 64, 32, 16, 8)                   # plan shapes 0 .. 4
SUB_SHIFT = {256: 0, 64: 0, 32: 1, 16: 2, 8: 3}
XTS = ("f64", "f32")
XDT = {"f64": np.float64, "f32": np.float32}
N_DST = 2 * 256 + 37                            # 549: the last block of every shape is partial
SEED = 20261017


def threads_of(shape):
    return 256 if shape == 256 else 64


def budget_of(shape):
    """Chunks a block may stage: 64 KiB of f64 per 4-wave block, 16 KiB per single wave."""
    return 2048 if shape == 256 else 512


def pieces_per_chunk(xt):
    """16-B staging pieces per 4-element chunk."""
    return 2 if xt == "f64" else 1


def np_class(np_needed):
    return 4 if np_needed <= 4 else (8 if np_needed <= 8 else 16)


# ------------------------------------------------------------------ the cell of a launch, from observable facts

def structural_cell(max_row, info, knobs):
    """The instantiation `launch_tile` runs, from `export_csr()`'s longest row, a `launch_info` dict and the knobs in
    force.  Returns (Cell, np_needed)."""
    assert info["kernel"] in ("tile", "tile-dma"), info
    shape, r = info["rows_per_block"], info["rows_per_step"]
    dma = info["kernel"] == "tile-dma"
    threads = threads_of(shape)
    np_needed, rem = divmod(info["lds_bytes"], r * (2 if dma else 1) * threads * 16)
    assert rem == 0 and 1 <= np_needed <= 16, info
    ss = SUB_SHIFT[shape]
    split = ss > 0 and knobs.get("tile_split_rows", 0) != 1 and max_row <= (48 << ss)
    if shape == 256:
        assert max_row <= 16
        maxk = 4 if max_row <= 4 else (8 if max_row <= 8 else 16)
    elif knobs.get("tile_links", 0) == 1:
        maxk = 0
    elif split:
        maxk = 32 if -(-max_row // (1 << ss)) <= 32 else 48
    else:
        maxk = 32 if max_row <= 32 else (48 if max_row <= 48 else 0)
    if dma:
        assert ss == 0 and maxk > 0 and (r == 1 or (maxk <= 16 and np_needed <= 4))
        n_p = np_class(np_needed)
    elif shape == 256 and r > 1:
        n_p = {4: 1, 2: 2}[r]               # the multi-row forms pin NP
    else:
        assert r == 1
        n_p = np_class(np_needed)
    return Cell(shape, maxk, n_p, r, "dma" if dma else "reg", bool(split and not dma), ss), np_needed


# ------------------------------------------------------------------ the cells the dispatcher can produce

def _reachable(xt):
    cells = set()
    for maxk in (4, 8, 16):                                      # 4-wave blocks
        for n_p, r in ((1, 4), (2, 2), (4, 1), (8, 1), (16, 1)):
            cells.add(Cell(256, maxk, n_p, r, "reg", False, 0))
        for n_p, r in ((4, 1), (4, 2), (4, 4), (8, 1), (16, 1)):
            cells.add(Cell(256, maxk, n_p, r, "dma", False, 0))
    for shape in (64, 32, 16, 8):                                # single-wave blocks
        ss = SUB_SHIFT[shape]
        for n_p in (4, 8, 16):
            for maxk in (32, 48, 0):
                cells.add(Cell(shape, maxk, n_p, 1, "reg", False, ss))
                cells.add(Cell(shape, maxk, n_p, 1, "dma", False, ss))
            for maxk in (32, 48):
                cells.add(Cell(shape, maxk, n_p, 1, "reg", True, ss))
    out = set()
    for c in cells:
        if c.split and c.sub_shift == 0:
            continue    # tile_split: sub_shift > 0
        if c.staging == "dma" and c.sub_shift > 0:
            continue    # tile_launch_cfg: c.dma needs a.sub_shift == 0
        if c.staging == "dma" and c.maxk == 0:
            continue    # tile_launch_cfg: c.dma needs max_row_nnz <= 48 (go_dma refuses MAXK 0)
        if c.staging == "dma" and c.shape == 256 and c.np == 16:
            continue    # tile_launch_cfg: c.dma needs 2 * tile <= 65536, a 4-wave tile of NP 16 is > 32 KiB
        if xt == "f32" and c.np == 16:
            continue    # ensure_plan: the chunk budget is 64 / 16 KiB of f64; an f32 chunk is one piece: np_needed <= 8
        if c.shape == 256 and c.maxk == 4 and c.np == (16 if xt == "f64" else 8):
            continue    # build_tile_plan: a block stages what its links touch, 256 rows x 4 links <= 1024 chunks
        if c.shape == 8 and c.maxk == 32 and not c.split and c.np == (16 if xt == "f64" else 8):
            continue    # build_tile_plan: 8 rows x 32 links <= 256 chunks (split rows hold up to 256 links each)
        out.add(c)
    return frozenset(out)


REACHABLE = {xt: _reachable(xt) for xt in XTS}


# ------------------------------------------------------------------ planner and launcher restated (prediction)

def plan_stats(rowptr, col, rows):
    """`build_tile_plan` + `tighten_tile_plan` + `ensure_plan` for blocks of `rows` destination rows:
    dict(valid, preferred, max_chunks, block_chunks)."""
    n_dst = rowptr.size - 1
    budget = budget_of(rows)
    nb = -(-n_dst // rows)
    nch, nln, ndist, links = (np.zeros(nb, np.int64) for _ in range(4))
    for b in range(nb):
        d0, d1 = b * rows, min(n_dst, (b + 1) * rows)
        cols = np.unique(col[rowptr[d0]:rowptr[d1]])
        links[b] = rowptr[d1] - rowptr[d0]
        ndist[b] = cols.size
        nch[b] = np.unique(cols // CHUNK).size
        nln[b] = np.unique(cols // 16).size
    nnz = int(rowptr[-1])
    direct = nch > budget
    valid = int(links[direct].sum()) * 4 <= nnz
    if valid:
        for cand in (budget // 8, budget // 4, budget // 2):
            if cand < 1 or cand >= nch[~direct].max(initial=0):
                continue
            demoted = (~direct) & (nch > cand)
            if int(links[direct | demoted].sum()) * 100 <= nnz:     # at most 1 % of the links go direct
                direct = direct | demoted
                break
    return dict(valid=valid, preferred=int(ndist.sum()) * 10 >= int(nln[~direct].sum()) * 16,
                max_chunks=int(nch[~direct].max(initial=0)), block_chunks=nch)


def native_plan(rowptr, col):
    """The operator's own plan shape (smm_operator_create) and its stats."""
    max_row = int(np.diff(rowptr).max(initial=0))
    if max_row <= 16:
        return 256, plan_stats(rowptr, col, 256)
    w_first = 1
    while w_first < 4 and max_row > (48 << (w_first - 1)):
        w_first += 1
    for w in list(range(w_first, 5)) + list(range(1, w_first)):
        st = plan_stats(rowptr, col, SHAPES[w])
        if st["valid"] and st["preferred"]:
            return SHAPES[w], st
    return 64, plan_stats(rowptr, col, 64)


def model_launch_info(shape, max_chunks, max_row, batch, xt, knobs):
    """`tile_launch_cfg` for a forced tile launch of `batch` rows of an aligned field: the `launch_info` dict."""
    walk, staging, rows_knob = (knobs.get(k, 0) for k in ("tile_walk", "tile_staging", "tile_rows_per_step"))
    assert walk > 0, "the cases pin tile_walk"
    jpb = min(batch, walk)
    threads = threads_of(shape)
    four = shape == 256
    np_needed = -(-max_chunks * pieces_per_chunk(xt) // threads)
    tile = max(np_needed, 1) * threads * 16
    rows = (4 if np_needed <= 1 else (2 if np_needed <= 2 else 1)) if four else 1
    while rows > 1 and (rows > jpb or (rows_knob > 0 and rows > rows_knob)):
        rows //= 2
    wanted = staging == 2 or (staging == 0 and four and np_needed <= 2)
    dma = wanted and SUB_SHIFT[shape] == 0 and 0 < max_row <= 48 and 2 * tile <= 65536
    if dma:
        rows = 1
        if four and np_needed <= 4:
            rows = rows_knob if rows_knob in (1, 2, 4) else (2 if np_needed <= 1 else 1)
        while rows > 1 and (rows > jpb or 2 * rows * tile > 65536):
            rows //= 2
    return {"kernel": "tile-dma" if dma else "tile", "j_per_block": jpb, "rows_per_step": rows,
            "rows_per_block": shape, "lds_bytes": (2 if dma else 1) * rows * tile}


# ------------------------------------------------------------------ deterministic builders

def _deal(rng, lens, cover, window):
    """Rows of one block.  Every column of `cover` (ascending) is linked: the columns are dealt to the rows in order,
    in proportion to the row lengths, so that the rows' windows move along the block's footprint; a row's other
    links are drawn next to its own share from `window` (ascending, holds `cover`), so no other chunk is touched."""
    total = int(lens.sum())
    if cover.size > total:                                   # a partial block: keep both ends of the footprint
        cover = np.concatenate([cover[:total - 1], cover[-1:]]) if total > 1 else cover[:total]
    cum = np.concatenate([[0], np.cumsum(lens)])
    start = cum * cover.size // max(total, 1)
    rows = []
    for r, ln in enumerate(lens):
        own = cover[start[r]:start[r + 1]]
        need = int(ln) - own.size
        assert need >= 0
        if need:
            at = int(np.searchsorted(window, cover[min(start[r], cover.size - 1)]))
            half = max(2 * int(ln), 16)
            lo = max(0, min(at - half, window.size - 2 * half))
            cand = np.setdiff1d(window[lo:lo + 2 * half], own)
            assert cand.size >= need, "window too small for the row"
            own = np.concatenate([own, rng.choice(cand, size=need, replace=False)])
        rows.append(np.sort(own))
    return rows


def _row_lengths(rng, n, k, need, first, last):
    """Row lengths of a block of n rows whose links must cover `need` columns: random in [k/2, k]; the first block's
    first row has exactly k links, the last (partial) block has a row of 0 and a row of 1 links."""
    lens = rng.integers(max(1, k // 2), k + 1, size=n)
    if first:
        lens[0] = k
    if last and n >= 3:
        lens[1], lens[2] = 0, 1
    elif lens.sum() < need:
        lens[:] = k
    return lens


def steer_params(chunks, cap, k):
    """(c, p) of the steered layout for a footprint of `chunks` = 4 c + p chunks per block: c lines of 16 columns
    shared by the blocks of a 64-row slice, p private columns on lines of their own.  ensure_plan prefers a plan
    whose blocks consume >= 1.6 columns per staged 128-B line: blocks of m times the rows hold 16 c + m p columns on
    c + m p lines, preferred iff m p <= 24 c.  12 c < p <= 24 c makes the requested shape the first preferred one
    (14 c <= p <= 22 c is asked for: the partial last block shifts the sums a little).
    None if the block's links (cap) cannot cover 16 c + p columns or a row of k links does not fit."""
    best = None
    for c in range(1, chunks // 16 + 1):
        p = chunks - 4 * c
        if not (14 * c <= p <= 22 * c) or 16 * c + p > cap or 16 * c + p < k:
            continue
        score = abs(p / c - 18.0)
        if best is None or score < best[0]:
            best = (score, c, p)
    return None if best is None else best[1:]


@functools.lru_cache(maxsize=None)
def banded_links(shape, k, chunks, steered=False, n_dst=N_DST, seed=SEED):
    """SCRIP links (1-based, shuffled) of a banded operator planned with blocks of `shape` rows: longest row exactly
    k links, every full block stages exactly `chunks` chunks.  Returns dict(n_src, n_dst, src, dst, w, sentinels):
    sentinels = the first element of block 0's first staged chunk and the last element of its last one.

    Dense layout: block b owns a window of `chunks` consecutive chunks, disjoint from its neighbours' (a block of
    twice the rows stages twice the chunks).  The shape follows from k: <= 16 links -> 256 rows; 17 .. 48 -> 64;
    49 .. 96 -> 32; 97 .. 192 -> 16; more -> 8 (smm_operator_create starts at the shape whose lane groups hold a row).
    Steered layout (rows of 17 .. 48 links on blocks of 32 / 16 / 8 rows): see `steer_params`."""
    rng = np.random.default_rng([seed, shape, k, chunks, int(steered)])
    nb = -(-n_dst // shape)
    rows, sentinels = [], None
    if steered:
        assert shape in (32, 16, 8) and 17 <= k <= 48
        c, p = steer_params(chunks, shape * k, k)
        per_slice = 64 // shape
        slice_lines = c + per_slice * p + 1
    else:
        assert chunks <= min(budget_of(shape), shape * k) and CHUNK * chunks >= k
        assert SHAPES[0 if k <= 16 else min(4, 1 + sum(k > (48 << i) for i in range(3)))] == shape
    end = 0
    for b in range(nb):
        n = min(shape, n_dst - b * shape)
        f = chunks if n == shape else max(1, chunks * n // shape)
        if steered:
            line0 = (b // per_slice) * slice_lines
            pb = p if n == shape else max(1, p * n // shape)
            priv = (line0 + c + (b % per_slice) * p + np.arange(pb)) * 16 + rng.integers(0, 16, size=pb)
            priv[-1] |= 15
            cover = np.concatenate([np.arange(line0 * 16, (line0 + c) * 16), priv])
            window = cover
        else:
            base = b * (chunks + 3)                       # windows three chunks apart: no shared chunk, odd alignment
            cover = (base + np.arange(f)) * CHUNK + rng.integers(0, CHUNK, size=f)
            cover[0] = base * CHUNK
            if f > 1:
                cover[-1] = (base + f) * CHUNK - 1
            else:
                cover = np.array([base * CHUNK, base * CHUNK + 3])
            window = np.arange(base * CHUNK, (base + f) * CHUNK)
        lens = _row_lengths(rng, n, k, cover.size, b == 0, n < shape)
        if n < shape:
            lens = np.minimum(lens, window.size // 2)     # the partial block's smaller footprint holds shorter rows
        assert n < shape or lens.sum() >= cover.size, "the block's links cannot cover its footprint"
        blk = _deal(rng, lens, cover, window)
        if b == 0:
            sentinels = (int(cover[0]), int(cover[-1]))
        rows += blk
        end = max(end, int(window[-1]) + 1)
    n_src = -(-end // 16) * 16 + 16
    dst = np.repeat(np.arange(n_dst), [r.size for r in rows])
    src = np.concatenate(rows)
    w = rng.uniform(-0.2, 1.0, size=src.size)
    zero = rng.random(src.size) < 0.02                    # a few exact zeros: links like any other
    zero[np.isin(src, sentinels) & (dst < shape)] = False
    w[zero] = 0.0
    perm = rng.permutation(src.size)
    out = dict(n_src=n_src, n_dst=n_dst, src=(src[perm] + 1).astype(np.int32), dst=(dst[perm] + 1).astype(np.int32),
               w=w[perm], sentinels=sentinels)
    for a in (out["src"], out["dst"], out["w"]):
        a.setflags(write=False)
    return out


def ragged_sell_links(seed=SEED):
    """The SELL batch-tiling test's operator: rows of 0 .. 40 links, n_dst = 500 (no multiple of 64)."""
    from tests.helpers import ragged_links
    src, dst, w = ragged_links(np.random.default_rng(seed), 4000, 500, max_len=40)
    return 4000, 500, src, dst, w


def sell_batch_rows(batch, knob):
    """`sell_batch_rows` of smm_launch.hpp: the SELL kernel's BT."""
    if batch >= 8 and knob == 8:
        return 8
    if batch >= 4 and knob != 2:
        return 4
    return 2 if batch >= 2 else 1


# BT -> (sell_batch_rows knob, batches BT k + r for k in 0 .. 2, r in 0 .. BT - 1 without B = 0)
SELL_BT = {bt: (knob, [bt * k + r for k in range(3) for r in range(bt) if bt * k + r > 0])
           for bt, knob in ((1, 0), (2, 2), (4, 0), (8, 8))}


# ------------------------------------------------------------------ the cases

def chunks_for(np_needed, shape, xt, low):
    """The smallest (low) or largest footprint in chunks that needs `np_needed` pieces per thread."""
    t, q = threads_of(shape), pieces_per_chunk(xt)
    return ((np_needed - 1) * t) // q + 1 if low else (np_needed * t) // q


def stepped(cell, batch, walk):
    """The cell a launch of `batch` rows lands in: rows per step halve until they fit the walk (R <= j_per_block)."""
    r = cell.r
    while r > 1 and r > min(batch, walk):
        r //= 2
    if r == cell.r:
        return cell
    if cell.staging == "dma":
        return cell._replace(r=r)
    return cell._replace(r=r, np={2: 2, 1: 4}[r])


# (tile_walk, batch) per R: B = 1; B = R - 1 (the dispatcher steps R down); a walk tail B = 2 j_per_block + 1;
# multiples of j_per_block that are no multiple of R.  R = 4 needs walks of 5 rows (a walk of 3 would step it down).
_WALK_BATCH = {1: ((3, 1), (5, 11), (3, 6)),
               2: ((3, 1), (5, 11), (3, 3), (5, 15)),
               4: ((5, 1), (5, 3), (5, 11), (5, 5), (5, 15))}


# np_needed values per NP class: both sides of 1 | 2, 2 | 3, 4 | 5, 8 | 9 and the largest legal tile.  (np_needed, low)
_NP_SINGLE = {4: ((4, False), (2, True)), 8: ((5, True), (8, False)), 16: ((9, True), (16, False))}
_K_OF = {4: (4, 3), 8: (5, 8), 16: (9, 16), 32: (17, 32), 48: (33, 48)}          # both sides of every MAXK threshold
_K_SPLIT = {(1, 32): (49, 64), (1, 48): (65, 96), (2, 32): (97, 128), (2, 48): (129, 192),
            (3, 32): (193, 256), (3, 48): (257, 300)}                            # per_grp on either side of 32


def _recipes(xt):
    """(cell, knobs, [(k, np_needed, low), ...], steered) for every reachable cell."""
    REG, DMA = 1, 2
    out = []
    for cell in sorted(REACHABLE[xt]):
        knobs = {"tile_staging": DMA if cell.staging == "dma" else REG}
        steered = False
        if cell.shape == 256:
            if cell.staging == "reg":
                nps = {(1, 4): ((1, False), (1, True)), (2, 2): ((2, True), (2, False)),
                       (4, 1): ((3, True), (4, False))}.get((cell.np, cell.r)) or _NP_SINGLE[cell.np]
            elif cell.np == 4:
                # DMA ring: one piece per thread takes two rows by itself; tile_rows_per_step picks 1 / 2 / 4, and
                # 2 x 16 KiB and 4 x 8 KiB tiles fill the 64 KiB ring exactly
                nps = {1: ((3, True), (4, False)), 2: ((1, False), (4, False)), 4: ((1, False), (2, False))}[cell.r]
                knobs["tile_rows_per_step"] = cell.r
            else:
                nps = _NP_SINGLE[cell.np]
            ks = _K_OF[cell.maxk]
        else:
            nps = _NP_SINGLE[cell.np]
            if cell.split:
                ks = _K_SPLIT[(cell.sub_shift, cell.maxk)]
            elif cell.sub_shift == 0:
                ks = _K_OF[cell.maxk] if cell.maxk else (20, 41)
                if cell.maxk == 0:
                    knobs["tile_links"] = 1                      # rows of > 48 links plan part-of-a-slice blocks
            elif cell.maxk == 0:
                ks = _K_SPLIT[(cell.sub_shift, 32)]              # rows too long for one lane's registers ...
                knobs["tile_split_rows"] = 1                     # ... with the split forms switched off
            else:
                ks = _K_OF[cell.maxk]
                knobs["tile_split_rows"] = 1
                steered = True
        variants = []
        for i, (npn, low) in enumerate(nps):
            chunks = chunks_for(npn, cell.shape, xt, low)
            for k in (ks[i % 2], ks[1 - i % 2]):
                if steered:
                    # 16 c + p columns to cover with shape * k links: the nearest footprint that can be steered
                    lo, hi = (chunks_for(npn, cell.shape, xt, side) for side in (True, False))
                    fit = [f for f in (range(lo, hi + 1) if low else range(hi, lo - 1, -1))
                           if steer_params(f, cell.shape * k, k)]
                    if fit:
                        variants.append((k, fit[0]))
                        break
                else:
                    f = min(chunks, cell.shape * k)
                    if f >= chunks_for(npn, cell.shape, xt, True) and CHUNK * f >= k:
                        variants.append((k, f))
                        break
        assert variants, f"no operator for {cell} ({xt})"
        out.append((cell, knobs, variants, steered))
    return out


def _make_cases():
    rot = np.random.default_rng(SEED)
    cases = []
    for xt in XTS:
        for cell, knobs, variants, steered in _recipes(xt):
            for n, (w, batch) in enumerate(_WALK_BATCH[cell.r]):
                k, chunks = variants[n % len(variants)]
                kn = dict(knobs, tile_walk=w, tile_x_loads=int(rot.integers(1, 3)))
                got = stepped(cell, batch, w)
                masked, area_min = ((False, 0.0), (True, 0.0), (True, 0.37), (False, 0.37))[int(rot.integers(4))]
                has_skipna = got.shape == 256 or (not got.split and got.maxk in (32, 48))     # tile_has_skipna
                skipna = bool(has_skipna and rot.random() < 0.4)
                yt = XTS[int(rot.integers(2))]
                npn = -(-chunks * pieces_per_chunk(xt) // threads_of(cell.shape))
                cid = (f"{xt}-{got.shape}-k{got.maxk}-np{got.np}-r{got.r}-{got.staging}"
                       f"{'-split' if got.split else ''}-K{k}-F{chunks}-B{batch}-w{w}")
                cases.append(Case(cid, (cell.shape, k, chunks, steered), xt, yt, tuple(sorted(kn.items())),
                                  masked, area_min, skipna, batch, got, npn))
    return cases


CASES = _make_cases()
