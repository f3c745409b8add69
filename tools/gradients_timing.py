"""What `gradients=True` costs: the source-gradient stencil (smm_gradients) and the K-column apply (smm_apply_cols)
against today's column-0 answer and against the "stacked" route, on r1440x721 -> r360x180 bicubic (`bic`, 4 weight
columns) and second-order conservative (`con2`, 3) weights, HBM-resident float64 rows.

One process per method, the legs interleaved step by step after a warm-up, device ms from HIP events, medians:
  gradients    smm_gradients alone, with the bytes per second it reaches against its floor -- one read of f and one
               write of every plane
  apply_cols   smm_apply_cols: the planes of all rows into a scratch that holds them, then the K-column gather; the
               gather alone is reported as apply_cols - gradients
  sell_col0    smm_apply with SMM_APPLY_KERNEL_SELL on column 0 of the same operator: today's answer, so
               apply_cols / sell_col0 is what the feature costs
  stacked      the route the K-column apply is defined by, given the planes: a device-to-device interleave of f and the
               planes into X[b, s * K + k] plus the existing apply on the stacked operator of K * S source cells;
               stacked_apply is that apply alone, a lower bound of the route.  The interleave is the library's own gather
               on a permutation operator (one link of weight 1 per cell of X) over rows that hold f and the planes side
               by side -- the library has no other strided device-to-device copy; the fields are finite and far below
               1e19, so fill and epilogue leave them alone.  Its bits are checked against apply_cols on step 0.
One JSON line per method, printed and appended to profiles/gradients_timing.jsonl.

  python tools/gradients_timing.py [--rows 64] [--steps 9] [--warmup 2] [--only bic,con2]
"""
import sys

import numpy as np

import benchlib
from bench_inputs import seeded_block

GRID = ("r1440x721", "r360x180")


def build(method):
    """(operator with columns, rule, stacked operator, the interleave's permutation operator) of one method"""
    from smmregrid_amd import GradientRule, SparseOperator, gridgen
    w = gridgen.generate_weights(*GRID, method=method)
    S, D = w.sizes["src_grid_size"], w.sizes["dst_grid_size"]
    src, dst, rm = w["src_address"].values, w["dst_address"].values, w["remap_matrix"].values
    K = rm.shape[1]
    op = SparseOperator(S, D, src, dst, rm, device=0, columns=True)
    s_src = ((src.astype(np.int64) - 1)[:, None] * K + np.arange(K)[None, :] + 1).astype(np.int32).ravel()
    stacked = SparseOperator(S * K, D, s_src, np.repeat(dst, K), np.ascontiguousarray(rm).ravel(), device=0)
    cell = np.arange(S * K, dtype=np.int64)      # cell s * K + k of X comes from column k * S + s of [f | planes]
    perm = SparseOperator(S * K, S * K, ((cell % K) * S + cell // K + 1).astype(np.int32), (cell + 1).astype(np.int32),
                          np.ones(S * K), device=0)
    return op, GradientRule.from_weights(w), stacked, perm


def bench(method, rows, steps, warmup):
    import ctypes
    from smmregrid_amd import DeviceArray, _lib, to_device
    op, rule, stacked, perm = build(method)
    S, D, K, P = op.n_src, op.n_dst, op.n_cols, rule.n_planes
    print(f"# {method}: S = {S}, D = {D}, {K} columns, nnz = {op.nnz}, {rows} rows", file=sys.stderr, flush=True)
    x = np.ascontiguousarray(np.tile(seeded_block(S, np.float64, nan=False), ((rows + 15) // 16, 1))[:rows])
    dx = to_device(x)
    g = DeviceArray((rows, P, S), np.float64)
    scratch = DeviceArray((rows * P * S * 8,), np.uint8)
    y_cols, y_0, y_s = (DeviceArray((rows, D), np.float64) for _ in range(3))
    X = DeviceArray((rows, S * K), np.float64)
    legs = {
        "gradients": lambda: op.gradients(dx, rule, out=g),
        "apply_cols": lambda: op.apply(dx, y=y_cols, gradients=rule, scratch=scratch),
        "sell_col0": lambda: op.apply(dx, y=y_0, flags=_lib.APPLY_KERNEL_SELL),
        "stacked_apply": lambda: stacked.apply(X, y=y_s, flags=_lib.APPLY_KERNEL_SELL),
    }
    # rows that hold f and the planes side by side: f copied in once, the planes computed in place
    Z = DeviceArray((rows, S * K), np.float64)
    for b in range(rows):
        _lib.call("smm_memcpy_d2d", ctypes.c_void_p(Z.ptr + b * S * K * 8), ctypes.c_void_p(dx.ptr + b * S * 8), S * 8, None)
    _lib.call("smm_gradients", rule.plan(0), ctypes.c_void_p(Z.ptr), _lib.SMM_F64, S * K, ctypes.c_void_p(Z.ptr + S * 8), S,
              S * K, rows, None)

    def route():
        perm.apply(Z, y=X)
        return stacked.apply(X, y=y_s, flags=_lib.APPLY_KERNEL_SELL)
    legs["stacked"] = route
    legs["interleave"] = lambda: perm.apply(Z, y=X)
    legs["stacked_apply"] = legs.pop("stacked_apply")      # behind the legs that fill X

    def check(leg, result):
        if leg == "stacked":
            if not benchlib.same_bits(y_s.to_host(), y_cols.to_host()):
                raise SystemExit(f"{method}: the stacked route and smm_apply_cols differ")

    times = benchlib.time_events(legs, steps, warmup, check=check)
    res = {"tool": "gradients_timing", "method": method, "grids": list(GRID), "rows": rows, "steps": steps, "columns": K,
           "nnz": op.nnz, **benchlib.summary(times, 4)}
    ms = res["ms"]
    floor_bytes = rows * S * (8 + P * 8)
    res["gradients_floor_bytes"] = floor_bytes
    res["gradients_gbps"] = round(floor_bytes / (ms["gradients"] * 1e-3) / 1e9, 1)
    res["gather_ms"] = round(ms["apply_cols"] - ms["gradients"], 4)
    res["apply_cols_over_sell_col0"] = round(ms["apply_cols"] / ms["sell_col0"], 2)
    res["stacked_over_gather"] = round(ms["stacked"] / max(res["gather_ms"], 1e-9), 2)
    res["stacked_apply_over_gather"] = round(ms["stacked_apply"] / max(res["gather_ms"], 1e-9), 2)
    for o in (op, stacked, perm):
        o.close()
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=9, warmup=2, only="bic,con2", out="gradients_timing.jsonl", cfg_rows=False)
    ap.add_argument("--rows", type=int, default=64)
    return ap


def main():
    args = benchlib.parse(parser(), least=7, why="medians need at least 7 steps")
    for method in benchlib.split(args.only):
        benchlib.emit(bench(method, args.rows, args.steps, args.warmup), args.out)


if __name__ == "__main__":
    main()
