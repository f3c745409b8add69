"""The CF encode rule on the CPU: what makes `CFEncode.encode` a reference, and what makes the inputs of
tests/cf_cases.py adequate for the bit-equality checks of tests/test_gpu_packed_out_exact.py.

* `CFEncode.encode` against an independent exact statement of the rule in rational arithmetic (`fractions`).
* Mutation adequacy of the generated inputs: every wrong-kernel model of cf_cases differs from the reference on at
  least one generated value of every non-dyadic rule, save the pairs of `IDENTICAL`, which are the same function on
  the rule's whole pool (asserted).
* The dyadic control: why fields made of multiples of 1/8 under a power-of-two scale cannot see a reciprocal multiply,
  a re-associated form or a float32 intermediate.
* encode(decode(q)) == q over the whole raw domain: what the decode -> encode check on the GPU relies on."""
import math
from fractions import Fraction

import numpy as np
import pytest

from smmregrid_amd import CFDecode
from tests import cf_cases as C

RULE_RAW = [(s, o, raw) for s, o in C.RULES for raw in C.RAWS]
IDS = [C.rule_id(*r) for r in RULE_RAW]

# (scale, offset, raw, model) that are the reference itself on the rule's whole pool.
#  - i_finite_on_t, every rule: t = (y - o) / s is finite only where y is, and where y is finite but t overflows, r = +-inf
#    is out of range: testing the finiteness of t marks exactly the values the reference marks.  No input can tell the
#    two apart, so no kernel written that way is wrong.
#  - a_reciprocal on (-0.0037, 101325.0) -> int16: the pool holds no value whose product with 1 / s rounds across a
#    rounding boundary of rint (uint16, whose range lies elsewhere on the axis, has four).
IDENTICAL = {(s, o, raw.name, "i_finite_on_t") for s, o in C.NON_DYADIC for raw in C.RAWS} \
    | {(-0.0037, 101325.0, "int16", "a_reciprocal")}


def exact_encode(y, scale, offset, raw):
    """The rule in exact arithmetic, rounded where the rule rounds: the difference of the two doubles rounded to
    double, its exact quotient by the scale rounded to double, that double rounded to an integer, ties to even."""
    info, fill = np.iinfo(raw), C.FILLS[np.dtype(raw)]
    if not math.isfinite(y):
        return fill
    d = float(Fraction(y) - Fraction(offset))            # int / int true division: correctly rounded
    t = float(Fraction(d) / Fraction(scale))
    r = round(Fraction(t))                               # Fraction.__round__: half to even, an exact int
    return r if info.min <= r <= info.max else fill


@pytest.mark.parametrize("scale,offset,raw", RULE_RAW, ids=IDS)
def test_encode_equals_the_exact_statement_of_the_rule(scale, offset, raw):
    cases = C.cases(scale, offset, raw)
    rng = np.random.default_rng(3)
    y = np.concatenate([C.SPECIALS, C.edges(scale, offset, raw), rng.choice(cases, 3000, replace=False)])
    got = C.reference(y, scale, offset, raw)
    assert got.dtype == raw
    want = np.array([exact_encode(float(v), scale, offset, raw) for v in y]).astype(raw)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(y[i]).hex(), int(got[i]), int(want[i])) for i in bad[:3]]
    fill = C.FILLS[np.dtype(raw)]
    assert (want == fill).any() and (want != fill).sum() > 2000


@pytest.mark.parametrize("scale,offset,raw", RULE_RAW, ids=IDS)
def test_case_sets_hold_what_they_promise(scale, offset, raw):
    cases = C.cases(scale, offset, raw)
    bits = cases.view(np.uint64)
    assert cases.ndim == 1 and cases.dtype == np.float64 and 10000 < cases.size <= C.MAX_CASES
    assert np.unique(bits).size == cases.size
    assert cases is C.cases(scale, offset, raw) and not cases.flags.writeable
    for must in (C.SPECIALS, C.edges(scale, offset, raw)):
        assert np.isin(must.view(np.uint64), bits).all()
    # the edges are one ulp apart and straddle the ends of the raw range
    info, fill = np.iinfo(raw), C.FILLS[np.dtype(raw)]
    e = C.edges(scale, offset, raw)
    assert np.array_equal(np.rint((e - offset) / scale), [info.max, info.max + 1, info.min - 1, info.min])
    assert all(np.nextafter(e[i], e[i + 1]) == e[i + 1] for i in (0, 2))
    # ties: all of the pool's where they fit, else as many as the edges, specials, fill values and the PER_MODEL
    # separating values per model leave room for
    with np.errstate(all="ignore"):
        t = (cases - offset) / scale
        ties = int((np.abs(t - np.floor(t)) == 0.5).sum())
    pinfo = C.pool_info(scale, offset, raw)
    assert ties >= (pinfo["ties"] if pinfo["all_ties"] else pinfo["tie_room"]), (ties, pinfo)
    assert pinfo["tie_room"] > C.MAX_CASES - 5000
    # valid values that round onto the fill value, from both sides of it where the range has two
    r = np.rint(t)
    assert (np.isfinite(cases) & (r == fill)).sum() >= 3
    # at least PER_MODEL separating values per model where the pool has that many
    counts = C.pool_counts(scale, offset, raw)
    for name, n_pool in counts.items():
        n = int(C.disagreements(name, cases, scale, offset, raw).sum())
        assert n >= min(n_pool, C.PER_MODEL), (name, n, n_pool)


@pytest.mark.parametrize("scale,offset,raw", [r for r in RULE_RAW if r[:2] != C.CONTROL],
                         ids=[i for r, i in zip(RULE_RAW, IDS) if r[:2] != C.CONTROL])
def test_every_wrong_kernel_model_is_caught_on_every_non_dyadic_rule(scale, offset, raw):
    cases = C.cases(scale, offset, raw)
    counts = C.pool_counts(scale, offset, raw)
    for name in C.MODELS:
        n = int(C.disagreements(name, cases, scale, offset, raw).sum())
        print(f"{C.rule_id(scale, offset, raw)} {name}: {n} of {cases.size} generated values separate it "
              f"({counts[name]} of the pool)")
        if (scale, offset, raw.name, name) in IDENTICAL:
            assert counts[name] == 0 and n == 0, (name, counts[name], n)
        else:
            assert n >= 1, name


@pytest.mark.parametrize("raw", C.RAWS, ids=["i16", "u16"])
def test_the_dyadic_control_cannot_see_a_reciprocal_a_reassociation_or_float32(raw):
    """Under a power-of-two scale 1 / s is exact and so are y * (1 / s) and (y - o) / s for every y of the pool: models
    (a) and (b) are the reference on the whole control set.  Model (c) is the reference on every value float32 holds
    exactly -- the multiples of 1/8 the fields of test_gpu_packed_out.py are made of, here every lattice point
    offset + (n + h) * scale -- and differs only on their ulp neighbours, which float32 rounds back onto the lattice
    (and onto its ties).  The rounding and range models stay visible on the control: ties are what it is for."""
    scale, offset = C.CONTROL
    cases = C.cases(scale, offset, raw)
    counts = C.pool_counts(scale, offset, raw)
    for name in ("a_reciprocal", "b_reassociated"):
        assert counts[name] == 0 and not C.disagreements(name, cases, scale, offset, raw).any(), name
    info = np.iinfo(raw)
    n = np.arange(info.min - 2, info.max + 3, dtype=np.float64)
    lattice = np.concatenate([offset + (n + h) * scale for h in (0.0, 0.5)])
    assert np.array_equal(lattice, lattice.astype(np.float32).astype(np.float64)) and np.array_equal(lattice * 8, np.rint(lattice * 8))
    for name in C.EXACT_ON_DYADIC:
        assert not C.disagreements(name, lattice, scale, offset, raw).any(), name
    with np.errstate(all="ignore"):
        in32 = cases[np.isfinite(cases) & (cases.astype(np.float32).astype(np.float64) == cases)]
    assert in32.size > 20000 and not C.disagreements("c_float32", in32, scale, offset, raw).any()
    for name in ("d_half_away", "e_truncate", "f_saturate", "g_wrap", "h_range_on_t"):
        assert C.disagreements(name, cases, scale, offset, raw).any(), name


# C.NO_F32_ROUND_TRIP is dropped from the float32 round trip and kept in float64; the test after this one records that
# it does fail.


ROUND_TRIPS = [(s, o, raw, dt) for s, o, raw in RULE_RAW for dt in (np.float32, np.float64)
               if not (dt == np.float32 and (s, o) in C.NO_F32_ROUND_TRIP)]


def _there_and_back(scale, offset, raw, dtype):
    info, fill = np.iinfo(raw), C.FILLS[np.dtype(raw)]
    q = np.arange(info.min, info.max + 1).astype(raw)
    assert q.size == 65536
    return q, C.reference(CFDecode(scale, offset, (fill,), dtype).decode(q), scale, offset, raw)


@pytest.mark.parametrize("scale,offset,raw,dtype", ROUND_TRIPS,
                         ids=[f"{C.rule_id(s, o, raw)}-{np.dtype(dt).name}" for s, o, raw, dt in ROUND_TRIPS])
def test_encode_of_decode_is_the_identity_on_the_whole_raw_domain(scale, offset, raw, dtype):
    q, back = _there_and_back(scale, offset, raw, dtype)
    assert back[q == C.FILLS[np.dtype(raw)]] == C.FILLS[np.dtype(raw)]        # NaN -> the fill value
    assert np.array_equal(back, q)


@pytest.mark.parametrize("raw", C.RAWS, ids=["i16", "u16"])
def test_the_rule_dropped_from_the_float32_round_trip_does_not_read_back(raw):
    for scale, offset in C.NO_F32_ROUND_TRIP:
        q, back = _there_and_back(scale, offset, raw, np.float32)
        assert (back != q).sum() > 1000
