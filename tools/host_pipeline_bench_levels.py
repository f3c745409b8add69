#!/usr/bin/env python3
"""Host-to-host rate of smm_group_apply_host on config-3 shaped fields (75 masked ocean levels,
1442x1021 -> r360x180 conservative): level-major packing of the used cells (round 6) against whole rows, with the
stage split of smm_debug_host_stats.   python tools/host_pipeline_bench_levels.py [time steps, default 16]"""
import argparse
import time

import numpy as np

import benchlib


def run(n_t, n_lev=75, nx=1442, ny=1021):
    from smmregrid_amd import _lib
    from smmregrid_amd.device import result_cache
    grp, masks, ml = benchlib.build_group(n_lev, nx, ny)
    rng = np.random.default_rng(0)
    slab = 10.0 + 5.0 * rng.standard_normal((n_lev, nx * ny))
    slab[masks == 0] = np.nan
    x = np.ascontiguousarray(np.broadcast_to(slab[None, :, None, :], (n_t, n_lev, 1, nx * ny)))
    lev = np.arange(n_lev, dtype=np.int32)
    out = {"time_steps": n_t, "levels": n_lev, "input_GB": x.nbytes / 1e9,
           "used_fraction": sum(op.n_used_src for op in grp.operators) / (n_lev * nx * ny)}
    ref = None
    for mode, fl in (("packed", 0), ("whole_rows", _lib.APPLY_HOST_NO_PACK)):
        y = grp.apply_host(x, lev, ml, masked=True, remap_area_min=0.5, flags=fl)      # warm-up
        y = None
        result_cache.wait()      # the steady state of a loop: the page-locked result block prepared in the background is there
        _lib.host_stats(reset=True)
        t0 = time.perf_counter()
        y = grp.apply_host(x, lev, ml, masked=True, remap_area_min=0.5, flags=fl)
        dt = time.perf_counter() - t0
        st = _lib.host_stats(reset=True)
        out[mode] = {"seconds": dt, "cells_per_s": n_t * n_lev * grp.n_dst / dt, "host_GBs": x.nbytes / dt / 1e9}
        out[mode]["stages"] = {k: round(v, 1) for k, v in st.items()}
        if ref is None:
            ref = y
        else:
            out["bit_identical"] = bool(np.array_equal(np.isnan(y), np.isnan(ref)) and
                                        np.array_equal(y[~np.isnan(y)], ref[~np.isnan(ref)]))
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("time_steps", type=int, nargs="?", default=16)
    return ap


if __name__ == "__main__":
    benchlib.emit(run(parser().parse_args().time_steps))
