"""The chunk loop of `apply_host_grib(ccsds=)` / `(cpx=)` / `(grib_out=GribEncode(..., ccsds=...))` cut by its byte
budget (chunk_rows=0 and more than one chunk): the free device memory the loop reads is made small enough for about three
rows a chunk, and the call must give the bits of the single-chunk call.  The plan itself is pinned on the CPU in
tests/test_grib_chunk_plan.py, whose cost formula this test takes."""
import numpy as np
import pytest

from smmregrid_amd import GribEncode, _lib, device
from tests.test_gpu_grib_ccsds import operator, same_bits
from tests.test_gpu_grib_ccsds_encode import same_field
from tests.test_grib_chunk_plan import D, call, costs

pytestmark = pytest.mark.gpu


def greedy(cost, target):
    """Rows per chunk: a chunk takes rows while their cost stays within the target, and at least one."""
    sizes, used = [0], 0
    for c in cost:
        if sizes[-1] and used + c > target:
            sizes.append(0)
            used = 0
        sizes[-1] += 1
        used += c
    return sizes


def spy(monkeypatch, free):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    monkeypatch.setattr(device, "mem_info", lambda: (free, free))
    return names


@pytest.mark.parametrize("kind", ["ccsds", "cpx"])
def test_a_small_budget_splits_the_call_and_keeps_its_bits(hip, kind, monkeypatch):
    """The 8-row "mixed" call: coded and simple-packed rows, a bitmap three rows share."""
    op = operator()
    assert op.n_dst == D
    desc, buf, rows, recs, bms, _ = call(f"{kind}-mixed")
    kw = {kind: recs, "bitmaps": bms}
    whole = {skipna: op.apply_host_grib(buf, rows, skipna=skipna, **kw) for skipna in (False, True)}
    cost = costs(f"{kind}-mixed")
    target = sum(cost[:3]) + cost[3] // 2               # three rows and half of the fourth
    sizes = greedy(cost, target)
    assert sizes[0] == 3 and len(sizes) > 1 and sum(sizes) == 8
    bounds = np.cumsum([0] + sizes)
    coded = np.flatnonzero(desc.is_coded(recs, rows))
    with_coded = sum(bool(((coded >= a) & (coded < b)).any()) for a, b in zip(bounds, bounds[1:]))
    assert with_coded > 1
    names = spy(monkeypatch, 4 * target + 3)            # the loop takes a quarter of the free memory
    for skipna in (False, True):
        del names[:]
        got = op.apply_host_grib(buf, rows, skipna=skipna, chunk_rows=0, **kw)
        assert names.count(desc.unpack_entry) == with_coded, (names.count(desc.unpack_entry), sizes)
        assert names.count("smm_apply_grib_na" if skipna else "smm_apply_grib_bm") == len(sizes)
        same_bits(got, whole[skipna], f"{kind} skipna={skipna} in chunks of {sizes}")


def test_a_small_budget_splits_the_ccsds_output_road_too(hip, monkeypatch):
    """CCSDS in, CCSDS out: beside the input's cost a row counts its simple-packed slot, the bound of its stream and 20 B
    per 8 destination cells of scratch."""
    op = operator()
    _, buf, rows, recs, bms, _ = call("ccsds-mixed")
    enc = GribEncode(np.array([16, 12, 9, 24, 32, 16, 7, 12], dtype=np.int32), 1, ccsds=True)
    kw = dict(bitmaps=bms, ccsds=recs, grib_out=enc, masked=True, remap_area_min=0.5)
    whole = op.apply_host_grib(buf, rows, **kw)
    offs, total = enc.layout(D, 8)
    slot = np.diff(np.append(offs, np.uint64(total))).astype(np.int64)
    cost = [c + int(s) + int(b) + (D // 8 + 1) * 20 for c, s, b in zip(costs("ccsds-mixed"), slot, enc.ccsds_bounds(D, 8))]
    target = sum(cost[:3]) + cost[3] // 2
    sizes = greedy(cost, target)
    assert sizes[0] == 3 and len(sizes) > 1
    names = spy(monkeypatch, 4 * target + 3)
    got = op.apply_host_grib(buf, rows, chunk_rows=0, **kw)
    assert names.count("smm_grib_aec_pack") == names.count("smm_grib_pack") == len(sizes)
    assert names.count("smm_grib_aec_unpack") > 1
    same_field(got, whole, f"CCSDS output in chunks of {sizes}")
