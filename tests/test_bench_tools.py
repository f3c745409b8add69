"""The instruments behind profiles/*.jsonl, checked without a GPU: tools/bench_inputs.py builds byte for byte what the
tools built before they shared it (digests in tests/golden/bench_tools_parent.json, recorded from the tools as they
were), its encoders write streams that the library's host decoders and the tests' independent decoders read back, the
leg timers of tools/benchlib.py run the legs in the order and number they say, every tool still has its command line,
and no tool grows a private copy of a shared piece again.
"""
import glob
import hashlib
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bench_tools_parent.json")
# S: even (pack12 writes pairs), no multiple of 32 (the last group / block is short), more than 4096 samples (a CCSDS
# stream crosses a reference-sample interval at J = 32, rsi = 128); R: more rows than distinct ones, no multiple of them
S, R = 8200, 6
SHARED = ("benchlib", "bench_inputs", "coded_benches")


def tool(name):
    """a module of tools/, imported the way the tools import each other: by its bare name, tools/ on sys.path"""
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    return importlib.import_module(name)


def tool_names():
    return sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tools", "*_bench.py"))) + \
        ["host_pipeline_bench_levels"]


def masks_2():
    from smmregrid_amd import gridgen
    return gridgen.synthetic_ocean_masks(70, 36, 2)


def digest(obj):
    """sha256 over a builder's return value: arrays by dtype, shape and bytes, containers walked in order"""
    h = hashlib.sha256()

    def walk(o):
        if isinstance(o, np.ndarray):
            h.update(f"a{o.dtype.str}{o.shape}".encode())
            h.update(np.ascontiguousarray(o).tobytes())
        elif isinstance(o, (bytes, bytearray)):
            h.update(b"b" + bytes(o))
        elif isinstance(o, dict):
            for k in sorted(o, key=str):
                h.update(f"k{k}".encode())
                walk(o[k])
        elif isinstance(o, (list, tuple)):
            h.update(f"l{len(o)}".encode())
            for v in o:
                walk(v)
        else:
            h.update(f"s{type(o).__name__}{o!r}".encode())
    walk(obj)
    return h.hexdigest()


def new_inputs():
    """every builder of tools/bench_inputs.py that needs no device, at the arguments the golden digests were taken at"""
    from smmregrid_amd.griblite import CCSDS, CPX
    b = tool("bench_inputs")
    masks = masks_2()
    q16 = np.random.default_rng(1).integers(0, 1 << 16, size=S, dtype=np.uint32)
    q12 = np.random.default_rng(2).integers(0, 1 << 12, size=S, dtype=np.uint32)
    smooth = b.smooth_field(S, 1, np.random.default_rng(7))
    present = np.random.default_rng(8).random(S) >= 0.3
    ccsds = b.make_coded_streams(CCSDS, S, R)
    return {"pack16": b.pack16(q16), "pack12": b.pack12(q12), "smooth_field": smooth, "smooth_field_complex_tool": smooth,
            "make_streams": b.make_streams(S, R, 0), "make_streams_D1_w16": b.make_streams(S, R, 1, widths=(16,)),
            "make_bitmap_streams": b.make_bitmap_streams(S, R),
            "make_level_streams_16": b.make_level_streams(masks, 2, 16), "make_level_streams_12": b.make_level_streams(masks, 2, 12),
            "coded_ccsds": ccsds[:4] + ccsds[5:],      # the CCSDS tool's builder returned no record parameters
            "coded_cpx": b.make_coded_streams(CPX, S, R),
            "source_ccsds": b.source(S, R, b.SEEDS["ccsds"]), "source_cpx": b.source(S, R, b.SEEDS["cpx"]),
            "encode_ccsds": b.encode_ccsds(smooth), "encode_complex": b.encode_complex(smooth),
            "encode_complex_mv": b.encode_complex_mv(smooth[present], present),
            "int16_rows": b.int16_rows(R, S), "int16_rows_out_tool": b.int16_rows(R, S), "int16_levels": b.int16_levels(masks, 2),
            "half_fields_2d": b.half_fields((R, S)), "half_fields_3d": b.half_fields((2, 2, S)),
            "seeded_block": b.seeded_block(S, np.float64, False), "seeded_block_nan": b.seeded_block(S, np.float64, True),
            "thinned": b.thinned(masks), "mv_streams": b.make_mv_streams(S, R),
            "plain_complex_streams": b.make_plain_complex_streams(S, R), "lonlat_messages": b.lonlat_messages(30, 72, 37)}


def options_of(ap):
    """{option names: default} of a parser; a path under the repository is kept from its last directory on"""
    out = {}
    for a in ap._actions:
        if a.dest == "help":
            continue
        default = a.default
        if isinstance(default, str) and os.path.isabs(default):
            default = "/".join(default.split(os.sep)[-2:])
        out["/".join(a.option_strings) or a.dest] = default
    return out


def tool_parser(name):
    return tool(name).parser()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ inputs
def test_every_builder_returns_the_bytes_it_returned_before(golden):
    got = {k: digest(v) for k, v in new_inputs().items()}
    assert sorted(got) == sorted(golden["inputs"])
    assert {k for k in got if got[k] != golden["inputs"][k]} == set()


def test_the_padded_buffer_is_the_bytes_and_zeros_up_to_four():
    b = tool("bench_inputs")
    for n in (0, 1, 4, 117, 8200):
        buf = np.arange(n, dtype=np.uint8) | 1
        out = b.padded(buf)
        assert out.size == (n + 3) // 4 * 4 and np.array_equal(out[:n], buf) and not out[n:].any()


def test_the_message_writer_writes_what_the_test_suite_s_encoder_writes():
    """bench_inputs.grib1_message is the lon/lat, no-bitmap case of tests/test_griblite.encode, kept apart because
    tools/ imports nothing from tests/: the two must not drift."""
    from tests.test_griblite import encode
    b = tool("bench_inputs")
    rng = np.random.default_rng(3)
    for ni, nj, nbits in ((72, 37, 16), (36, 19, 12), (1440, 721, 16)):
        field = 250.0 + 30.0 * rng.standard_normal((nj, ni))
        date = (2021, 2, 27, 12)
        want = encode(field, 0, ni, nj, 90, 0, -90, 360.0 - 360.0 / ni, 180000 // (nj - 1), param=167, date=date, nbits=nbits)
        assert b.grib1_message(field, ni, nj, date, nbits=nbits) == want


@pytest.mark.parametrize("case, direct", [("cfg2", "bilinear_weights"), ("cfg5", "conservative_weights"),
                                          (("r70x36", "r36x18", "con"), "conservative_weights")])
def test_build_operator_s_weights_are_those_the_tools_generated_directly(case, direct):
    """half_bench, packed_bench and packed_out_bench called gridgen.bilinear_weights / conservative_weights themselves;
    benchlib.build_operator goes through gridgen.generate_weights for every case"""
    from smmregrid_amd import gridgen
    lib = tool("benchlib")
    sgrid, tgrid, method = lib.GRIDS.get(case, case) if isinstance(case, str) else case
    a, b = gridgen.generate_weights(sgrid, tgrid, method=method), getattr(gridgen, direct)(sgrid, tgrid)
    assert a.sizes["src_grid_size"] == b.sizes["src_grid_size"] and a.sizes["dst_grid_size"] == b.sizes["dst_grid_size"]
    for name in ("src_address", "dst_address", "remap_matrix"):
        assert np.array_equal(a[name].values, b[name].values), name


# ------------------------------------------------------------------------------------------------ encoders
@pytest.fixture(scope="module")
def smooth():
    b = tool("bench_inputs")
    rng = np.random.default_rng(20261019)
    return [b.smooth_field(S, i, rng) for i in range(2)]


def test_encode_ccsds_is_read_back_by_the_host_decoder_and_by_libaec(smooth):
    from tests import ccsds_cases
    b = tool("bench_inputs")
    for q in smooth:
        stream = b.encode_ccsds(q)
        assert np.array_equal(ccsds_cases.host_decode(stream, S, b.NBITS, b.BLOCK, b.RSI, b.FLAGS), q)
        # tests/ccsds_cases.py holds no decoder of its own: the independent reader of the format is libaec, and without
        # it this test fails rather than pass on the library's word alone
        assert ccsds_cases.load_libaec() is not None, "libaec not found (SMM_LIBAEC names it): no independent CCSDS decoder"
        assert np.array_equal(ccsds_cases.aec_decode_libaec(stream, S, b.NBITS, b.BLOCK, b.RSI, True), q)


def test_encode_complex_is_read_back_by_the_host_decoder_and_the_numpy_decoder(smooth):
    from smmregrid_amd.griblite import CPX, cpx_decode
    from tests import complex_cases
    b = tool("bench_inputs")
    for q in smooth:
        stream, p = b.encode_complex(q)
        assert p[0] == (S + 31) // 32 and p[6] == S % 32                 # a short last group
        assert np.array_equal(cpx_decode(stream, b.coded_record(CPX, 0, stream, S, p)), q)
        assert np.array_equal(complex_cases.numpy_decode(stream, S, dict(zip(complex_cases.PARAM_NAMES, p))), q)


@pytest.mark.parametrize("mvm", [1, 2])
def test_encode_complex_mv_is_read_back_with_its_presence_flags(smooth, mvm):
    from smmregrid_amd.griblite import CPX, cpx_decode_mv
    from tests import complex_cases, complex_mv_cases
    b = tool("bench_inputs")
    present = np.random.default_rng(8).random(S) >= b.MISSING
    q = smooth[0][present]
    stream, p = b.encode_complex_mv(q, present, mvm=mvm)
    got, there = cpx_decode_mv(stream, b.coded_record(CPX, 0, stream, S, p), mvm)
    assert np.array_equal(got, q) and np.array_equal(there, present)
    got, there = complex_mv_cases.numpy_decode(stream, S, dict(zip(complex_cases.PARAM_NAMES, p)), mvm)
    assert np.array_equal(got, q) and np.array_equal(there, present)


# ------------------------------------------------------------------------------------------------ timers
class Log:
    """fake legs, host_stats and events that write down what happened"""

    def __init__(self):
        self.calls = []

    def legs(self, *names):
        return {n: (lambda n=n: self.calls.append(("leg", n)) or n.upper()) for n in names}

    def host_stats(self, reset=False):
        self.calls.append(("stats", reset))
        return {"n": sum(1 for c in self.calls if c[0] == "leg")}

    def event(self):
        log = self

        class Event:
            def record(self):
                log.calls.append(("record", id(self)))

            def synchronize(self):
                log.calls.append(("sync", id(self)))

            def elapsed_ms(self, other):
                log.calls.append(("elapsed", id(self), id(other)))
                return 1.5
        return Event

    def order(self):
        return [c[1] for c in self.calls if c[0] == "leg"]


@pytest.mark.parametrize("timer", ["wall", "events"])
def test_legs_run_in_the_given_order_and_the_warm_up_is_dropped(timer):
    lib, log = tool("benchlib"), Log()
    run = (lambda **kw: lib.time_wall(log.legs("a", "b", "c"), 5, 2, **kw)) if timer == "wall" else \
        (lambda **kw: lib.time_events(log.legs("a", "b", "c"), 5, 2, event=log.event(), **kw))
    times = run()
    assert log.order() == ["a", "b", "c"] * 7
    assert list(times) == ["a", "b", "c"] and all(len(v) == 5 and all(t >= 0 for t in v) for v in times.values())


@pytest.mark.parametrize("timer", ["wall", "events"])
def test_both_orders_reverses_the_odd_steps(timer):
    lib, log = tool("benchlib"), Log()
    legs = log.legs("a", "b", "c")
    times = lib.time_wall(legs, 6, 1, both_orders=True) if timer == "wall" else \
        lib.time_events(legs, 6, 1, both_orders=True, event=log.event())
    assert log.order() == (["a", "b", "c"] + ["c", "b", "a"]) * 3 + ["a", "b", "c"]
    assert all(len(v) == 6 for v in times.values())
    marked = {k: [10 * i + j for i in range(6)] for j, k in enumerate(times)}       # timed step i is step 1 + i
    fwd, rev = lib.by_order(marked, 1)
    assert fwd["a"] == [10, 30, 50] and rev["a"] == [0, 20, 40]                      # steps 2, 4, 6 and 1, 3, 5


@pytest.mark.parametrize("timer", ["wall", "events"])
def test_the_callbacks_of_step_0(timer):
    lib, log = tool("benchlib"), Log()
    legs = log.legs("a", "b")
    seen = []
    kw = dict(after_first=lambda: log.calls.append(("after_first",)), check=lambda leg, res: seen.append((leg, res, len(log.order()))))
    lib.time_wall(legs, 5, 1, **kw) if timer == "wall" else lib.time_events(legs, 5, 1, event=log.event(), **kw)
    marks = [i for i, c in enumerate(log.calls) if c == ("after_first",)]
    assert len(marks) == 1                                                           # once ...
    before = [c[1] for c in log.calls[:marks[0]] if c[0] == "leg"]
    assert before == ["a", "b"]                                                      # ... behind every leg of step 0
    assert seen == [("a", "A", 1), ("b", "B", 2)]              # each leg's result, right behind it, in step 0 only


def test_host_stats_is_reset_before_and_read_after_every_leg():
    lib, log = tool("benchlib"), Log()
    times, stats = lib.time_wall(log.legs("a", "b"), 5, 1, host_stats=log.host_stats)
    per_leg = [log.calls[i:i + 3] for i in range(0, len(log.calls), 3)]
    assert len(per_leg) == 12 and all(c[0] == ("stats", True) and c[1][0] == "leg" and c[2] == ("stats", True) for c in per_leg)
    assert [s["n"] for s in stats["a"]] == [3, 5, 7, 9, 11] and [s["n"] for s in stats["b"]] == [4, 6, 8, 10, 12]
    assert all(len(v) == 5 for v in times.values())


def test_the_event_timer_records_calls_records_and_synchronises_the_second_event():
    lib, log = tool("benchlib"), Log()
    times = lib.time_events(log.legs("a"), 5, 1, event=log.event())
    kinds = [c[0] for c in log.calls]
    assert kinds[:4] == ["record", "leg", "record", "sync"]                          # a warm-up step: no elapsed_ms
    assert kinds[4:9] == ["record", "leg", "record", "sync", "elapsed"]
    first, second = log.calls[4][1], log.calls[6][1]
    assert first != second and log.calls[7] == ("sync", second) and log.calls[8] == ("elapsed", first, second)
    assert times == {"a": [1.5] * 5}


def test_summary_and_median():
    lib = tool("benchlib")
    times = {"a": [3.0004, 1.0, 2.0], "b": [4.0, 4.0]}
    assert lib.median(times["a"]) == 2.0
    assert lib.summary(times, 3) == {"ms": {"a": 2.0, "b": 4.0}, "ms_min": {"a": 1.0, "b": 4.0}}
    assert lib.summary(times, 3, maximum=True)["ms_max"] == {"a": 3.0, "b": 4.0}


def test_fewer_than_five_steps_are_refused(capsys):
    lib = tool("benchlib")
    ap = lib.parser("doc", steps=7, warmup=2, only="cfg2,cfg4", blocks="host,kernel", out="x.jsonl")
    assert lib.parse(ap, []).steps == 7 and lib.parse(ap, ["--steps", "5"]).steps == 5
    with pytest.raises(SystemExit):
        lib.parse(ap, ["--steps", "4"])
    assert "median and best need at least 5 timings" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        lib.parse(ap, ["--steps", "7"], least=6, both_orders=True, why="an even number")


def test_emit_prints_and_appends(tmp_path, capsys):
    lib = tool("benchlib")
    path = tmp_path / "made" / "x.jsonl"
    lib.emit({"a": 1}, str(path))
    lib.emit({"b": 2}, str(path))
    lib.emit({"c": 3})
    assert capsys.readouterr().out.splitlines() == ['{"a": 1}', '{"b": 2}', '{"c": 3}']
    assert path.read_text().splitlines() == ['{"a": 1}', '{"b": 2}']


# ------------------------------------------------------------------------------------------------ command lines
def test_every_tool_keeps_its_options_and_defaults(golden):
    # tools/user_path_bench.py reads sys.argv itself ([rows] [--only-h2h] [knob=value ...]) and did not change
    names = [n for n in tool_names() if n != "user_path_bench"]
    assert sorted(names) == sorted(golden["cli"])
    for name in names:
        assert options_of(tool_parser(name)) == golden["cli"][name], name


# ------------------------------------------------------------------------------------------------ structure
def _sources():
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        if os.path.basename(path)[:-3] not in SHARED[:2]:
            with open(path) as f:
                yield os.path.basename(path), f.read()


def test_no_tool_defines_a_shared_piece_of_its_own():
    pattern = re.compile(r"^\s*def (_median|median|smooth_field|make_streams|encode_ccsds|encode_complex\w*)\(", re.M)
    assert {name: pattern.findall(src) for name, src in _sources() if pattern.search(src)} == {}


def test_no_tool_imports_another_tool():
    pattern = re.compile(r"importlib\.util|from tools\.\w+_bench import|import \w+_bench\b|from tools import \w+_bench\b")
    assert {name: pattern.findall(src) for name, src in _sources() if pattern.search(src)} == {}


def test_no_bench_tool_imports_from_the_tests():
    # the bench tools and their shared modules; tools/soak.py draws its operators from the test suite on purpose
    mine = {n + ".py" for n in tool_names() + list(SHARED)}
    for name in sorted(mine):
        with open(os.path.join(ROOT, "tools", name)) as f:
            assert not re.search(r"^\s*(from|import) tests\b", f.read(), re.M), name
