"""The harness of the tools/*_bench.py tools: importing it puts the repository root on sys.path, and it holds the one
definition of everything the tools share beside their inputs (tools/bench_inputs.py) -- the median and the summary of
the timings, the wall-clock and the HIP-event leg timers, the operators and the level group, the shared command-line
options and the "print and append a JSON line" tail.  Plain functions; a published figure depends on where these loops
synchronise and in which order they run the legs, so tests/test_bench_tools.py pins both with fake legs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = ("stage_in_ms", "h2d_ms", "kernel_ms", "d2h_ms", "copy_out_ms", "wait_ms", "chunks")
GRIDS = {"cfg2": ("r1440x721", "r360x180", "bil"), "cfg4": ("n1280", "hp1024", "bil"), "cfg5": ("r1440x721", "r720x360", "con")}


def median(v):
    return float(np.median(np.asarray(v)))


def summary(times, digits, maximum=False):
    """{leg: [ms]} -> {"ms": medians, "ms_min": the best (, "ms_max": the worst)} rounded to `digits`"""
    out = {"ms": {k: round(median(v), digits) for k, v in times.items()},
           "ms_min": {k: round(min(v), digits) for k, v in times.items()}}
    if maximum:
        out["ms_max"] = {k: round(max(v), digits) for k, v in times.items()}
    return out


def stage_split(stats):
    """the medians of the pipeline's stages over the host_stats of a leg's timed steps"""
    return {n: round(median([st[n] for st in stats]), 3) for n in STAGES}


# ------------------------------------------------------------------------------------------------ the leg timers
def _run_legs(legs, steps, warmup, timed, after_first, check, both_orders, announce):
    """The one loop: the legs interleaved step by step -- in the order given, reversed on odd steps under both_orders --
    for warmup + steps steps, the warm-up steps' timings dropped.  timed(leg, fn, keep) -> (ms, fn's result).
    check(leg, result) runs behind every leg of step 0, after_first() once behind step 0."""
    names = list(legs)
    times = {k: [] for k in names}
    for step in range(warmup + steps):
        if announce:
            print(announce.format(step), file=sys.stderr, flush=True)
        for leg in (names[::-1] if both_orders and step % 2 else names):
            ms, result = timed(leg, legs[leg], step >= warmup)
            if step >= warmup:
                times[leg].append(ms)
            if step == 0 and check:
                check(leg, result)
        if step == 0 and after_first:
            after_first()
    return times


def time_wall(legs, steps, warmup, host_stats=None, after_first=None, check=None, both_orders=False, announce=None):
    """Wall-clock ms of {leg: callable}: time.perf_counter around each call.  host_stats: `_lib.host_stats`, reset before
    and read after every leg; the result is then (times, {leg: [the stats of its timed steps]}).  announce: a line with
    one {} for the step number, written to stderr ahead of every step."""
    stats = {k: [] for k in legs}

    def timed(leg, fn, keep):
        if host_stats:
            host_stats(reset=True)
        t0 = time.perf_counter()
        result = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if host_stats:
            st = host_stats(reset=True)
            if keep:
                stats[leg].append(st)
        return ms, result
    times = _run_legs(legs, steps, warmup, timed, after_first, check, both_orders, announce)
    return (times, stats) if host_stats else times


def time_events(legs, steps, warmup, after_first=None, check=None, both_orders=False, event=None):
    """Device ms of {leg: callable} from HIP events: record e0, call the leg, record e1, synchronise e1 -- per leg, per
    step.  event: the event class (smmregrid_amd.device.Event)."""
    if event is None:
        from smmregrid_amd.device import Event as event
    e0, e1 = event(), event()

    def timed(leg, fn, keep):
        e0.record()
        result = fn()
        e1.record()
        e1.synchronize()
        return (e0.elapsed_ms(e1) if keep else 0.0), result
    return _run_legs(legs, steps, warmup, timed, after_first, check, both_orders, None)


def by_order(times, warmup):
    """({leg: the timings of the even steps}, {leg: those of the odd steps}) of a both_orders run"""
    fwd = {k: [t for i, t in enumerate(v) if (warmup + i) % 2 == 0] for k, v in times.items()}
    rev = {k: [t for i, t in enumerate(v) if (warmup + i) % 2] for k, v in times.items()}
    return fwd, rev


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def time_calls(fn, steps):
    """wall-clock ms of `steps` calls of fn, one after the other (the host decodes timed on their own)"""
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def median_and_min(times, digits=3):
    return {"median": round(median(times), digits), "min": round(min(times), digits)}


def time_decode_rule(buf, rule, bm, S, steps):
    """griblite's decode of one bitmapped message, as open_grib runs it, with the float32 store"""
    from smmregrid_amd.griblite import _decode_rule
    row = np.empty(S, dtype=np.float32)

    def decode():
        row[:] = _decode_rule(buf, rule, S, bm)
    return time_calls(decode, steps)


def time_level_decode(buf, first, S, steps):
    """The same for one message per level (`first`: each level's rule and bitmap): the median per level, summed over
    the levels = one time step of the variable"""
    return sum(median(time_decode_rule(buf, rule, bm, S, steps)) for rule, bm in first)


# ------------------------------------------------------------------------------------------------ operators
def build_operator(case, device=0):
    """The SparseOperator of "cfg2" (bilinear r1440x721 -> r360x180), "cfg4" (bilinear n1280 -> hp1024), "cfg5" (the
    conservative r1440x721 -> r720x360 of config 5's geometry) or of a (source grid, target grid, method) of one's own."""
    from smmregrid_amd import SparseOperator, gridgen
    sgrid, tgrid, method = GRIDS.get(case, case) if isinstance(case, str) else case
    w = gridgen.generate_weights(sgrid, tgrid, method=method)
    return SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                          w["dst_address"].values, w["remap_matrix"].values, device=device)


def build_group(n_lev, nx=1440, ny=721, target="r360x180", device=0):
    """(OperatorGroup, the levels' source masks, masked_levels) of conservative weights per level on synthetic ocean
    masks of an nx x ny regular grid"""
    from smmregrid_amd import OperatorGroup, gridgen
    from smmregrid_amd.weights import compute_weights_matrix3d
    masks = gridgen.synthetic_ocean_masks(nx, ny, n_lev)
    w3 = gridgen.ConservativeLevels(gridgen.regular_grid(nx, ny), target).stack(masks, np.arange(n_lev, dtype=np.float64))
    ops = compute_weights_matrix3d(w3, "lev", device=device)
    imask = np.stack([op.mask_apply(masks[i]) for i, op in enumerate(ops)])
    for i, op in enumerate(ops):
        op.set_epilogue(imask[i], w3["dst_grid_frac"].values[i])
    return OperatorGroup(ops), masks, (~(imask == 1).all(axis=1)).astype(np.uint8)


def one_link_operator(n_src):
    """an operator of the same source grid with ONE link: a GRIB call on it is the table build and next to no gather"""
    from smmregrid_amd import SparseOperator
    return SparseOperator(n_src, 1, np.array([1]), np.array([1]), np.array([1.0]), device=0)


# ------------------------------------------------------------------------------------------------ command line, output
def parser(doc, steps, warmup, only=None, blocks=None, out=None, cfg_rows=True, steps_help=None):
    """An ArgumentParser with the options the tools share: --steps, --warmup and, where a default is given, --only,
    --blocks and --out (a file name under profiles/); cfg_rows: --cfg4-rows 128 and --cfg2-rows 512."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    if cfg_rows:
        ap.add_argument("--cfg4-rows", type=int, default=128)
        ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=steps, help=steps_help)
    ap.add_argument("--warmup", type=int, default=warmup)
    if only is not None:
        ap.add_argument("--only", default=only)
    if blocks is not None:
        ap.add_argument("--blocks", default=blocks)
    if out is not None:
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    return ap


def parse(ap, argv=None, least=5, why="median and best need at least 5 timings", both_orders=False):
    """The arguments, refused with `why` below `least` timed steps; both_orders: the steps and the warm-up must be even
    too, so that both orders get the same share."""
    args = ap.parse_args(argv)
    if args.steps < least or (both_orders and (args.steps % 2 or args.warmup % 2)):
        ap.error(why)
    return args


def split(text):
    return [v.strip() for v in text.split(",")]


def operators(args, announce=True):
    """(name, operator, rows) of every case of --only, built in turn and closed behind the caller's loop body"""
    for name in split(args.only):
        op, rows = build_operator(name), {"cfg4": args.cfg4_rows, "cfg2": args.cfg2_rows}[name]
        if announce:
            print(f"# {name}: operator built (S = {op.n_src}, D = {op.n_dst}), {rows} rows", file=sys.stderr, flush=True)
        yield name, op, rows
        op.close()


def emit(res, path=None):
    """Print the JSON line; with a path, append it to that file (its directory is made)."""
    line = json.dumps(res)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")
