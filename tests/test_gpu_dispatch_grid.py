"""The whole (x_dtype, y_dtype, decode_dtype, skipna) grid through the six `_pk` entries: every combination the header
documents as built gives the bits of host decode -> CPU oracle -> host encode, every other one its documented refusal
with Y untouched.

The CPU side: `CFDecode.decode` (the host decode), `oracle.apply_c` (plain) or `tests.helpers.skipna_ref` (the skipna
rule, which the oracle does not carry) on that field in float64, a cast for float32 results, `CFEncode.encode` for
packed ones -- the helpers of tests/test_gpu_packed*.py and tests/test_gpu_skipna.py.

Shapes: 70 source cells of which 50 carry links (the host pipelines pack such an operator from 8 rows per chunk on),
130 destination cells (past one 64-row SELL slice and a ragged last tile for every batch-fastest tile height 16 / 32 /
64), batches of 3 and 130 (both sides of the 128-entry batch tile and of the SELL batch-rows choice), a two-level group
read through level_index [1, 0] with the mask of one member switched off.  The host entries run with the library's
own chunks and with three chunks, so that the pipeline reuses a buffer."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import CFDecode, CFEncode, OperatorGroup, SparseOperator, _lib, to_device
from tests.helpers import random_links, skipna_ref

pytestmark = pytest.mark.gpu
S, S_USED, D, L = 70, 50, 130, 2
BATCHES = (3, 130)
LEV = np.array([1, 0], dtype=np.int32)             # data level -> group member
MASKED_LEVELS = np.array([1, 0], dtype=np.uint8)   # per member: member 1 ignores its mask
AREA_MIN = 0.5
F32, F64, I16, U16 = _lib.SMM_F32, _lib.SMM_F64, _lib.SMM_I16, _lib.SMM_U16
NP = {F32: np.dtype(np.float32), F64: np.dtype(np.float64), I16: np.dtype(np.int16), U16: np.dtype(np.uint16)}
NAME = {F32: "f32", F64: "f64", I16: "i16", U16: "u16"}
UNS = _lib.SMM_ERR_UNSUPPORTED
# (x_dtype, y_dtype) -> None (built) or (status, a word of the message); include/smmregrid_amd.h: float fields give
# float or packed results; a packed field gives SMM_F64 (SMM_F32 "is not built") or packed results of its own raw type
STATUS = {
    (F32, F32): None, (F32, F64): None, (F32, I16): None, (F32, U16): None,
    (F64, F32): None, (F64, F64): None, (F64, I16): None, (F64, U16): None,
    (I16, F32): (UNS, b"not built"), (I16, F64): None, (I16, I16): None, (I16, U16): (UNS, b"own raw type"),
    (U16, F32): (UNS, b"not built"), (U16, F64): None, (U16, I16): (UNS, b"own raw type"), (U16, U16): None,
}
SENTINEL = 0x5A


def decode_rule(raw, decode):
    """The rules of tests/test_gpu_packed_levels.py: a float32 decode that rounds / a negative scale; two fills each."""
    if np.dtype(raw) == np.int16:
        return CFDecode(1.9e-3, 2.7e2, (-32768, 7), decode)
    return CFDecode(-0.25, 12.5, (65535, 300), decode)


def encode_rule(raw):
    """Rows hold up to a dozen weights within (-0.5, 1.5): results of the int16 field stay within a few thousand, those
    of the uint16 field (values down to -16371) reach beyond the raw range now and then -- these become the fill."""
    if np.dtype(raw) == np.int16:
        return CFEncode(0.25, 1000.0, -32768, np.int16)
    return CFEncode(2.0, -60000.0, 65535, np.uint16)


@functools.lru_cache(maxsize=None)
def geometry():
    rng = np.random.default_rng(1807)
    ops, csrs, imasks, fracs = [], [], [], []
    for _ in range(L):
        src, dst, w = random_links(rng, S_USED, D, 600)
        op = SparseOperator(S, D, src, dst, w, device=0)
        imask = (rng.random(D) < 0.8).astype(np.int32)
        frac = rng.random(D)
        op.set_epilogue(imask, frac)
        ops.append(op)
        csrs.append(op.export_csr())
        imasks.append(imask)
        fracs.append(frac)
    assert ops[0].n_used_src * 5 <= S * 4 and ops[0].max_row_nnz <= 16
    return {"ops": ops, "grp": OperatorGroup(ops), "csrs": csrs, "imask": imasks, "frac": fracs}


@functools.lru_cache(maxsize=None)
def raw_field(raw_name, batch):
    """(batch, L, S) raw values over the whole range of the type, either fill value on 3 % of the cells."""
    rng = np.random.default_rng(97 + batch)
    info, fills = np.iinfo(raw_name), decode_rule(raw_name, np.float32).fill_values
    q = rng.integers(info.min, info.max + 1, size=(batch, L, S)).astype(raw_name)
    for f in fills:
        q[q == f] = f + 1 if f < info.max else f - 1
    scattered = rng.random(q.shape) < 0.03
    q[scattered] = np.where(rng.random(int(scattered.sum())) < 0.5, fills[0], fills[-1]).astype(raw_name)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def inputs(x_dtype, decode_dtype, batch):
    """(the field the entries get, (batch, L, S); its CFDecode or None; the host-decoded field the CPU side regrids).
    A float field is the int16 field decoded on the host in that float type."""
    if x_dtype in (I16, U16):
        q = raw_field(NP[x_dtype].name, batch)
        cf = decode_rule(NP[x_dtype], NP[decode_dtype])
        return q, cf, cf.decode(q)
    x = decode_rule(np.int16, NP[x_dtype]).decode(raw_field("int16", batch))
    assert x.dtype == NP[x_dtype]
    return x, None, x


@functools.lru_cache(maxsize=None)
def expectation(x_dtype, decode_dtype, skipna, batch):
    """float64 (batch, L, D): host decode -> CPU oracle per data level; computed once, read-only."""
    g = geometry()
    xv = inputs(x_dtype, decode_dtype, batch)[2]
    out = np.empty((batch, L, D))
    for l in range(L):
        m = int(LEV[l])
        masked = bool(MASKED_LEVELS[m])
        xl = np.ascontiguousarray(xv[:, l])
        if skipna:
            out[:, l] = skipna_ref(g["csrs"][m], xl, masked, g["imask"][m], g["frac"][m], AREA_MIN)
        else:
            out[:, l] = oracle.apply_c(g["csrs"][m], xl, masked, g["imask"][m], g["frac"][m], AREA_MIN)
    share = float(np.isnan(out).mean())
    assert 0.05 <= share <= 0.9, share          # the masks, the fills and remap_area_min all bite, and not everywhere
    out.setflags(write=False)
    return out


def as_result(y64, y_dtype):
    if y_dtype in (I16, U16):
        return encode_rule(NP[y_dtype]).encode(y64)
    return y64.astype(NP[y_dtype])


@functools.lru_cache(maxsize=None)
def device_inputs(x_dtype, decode_dtype, batch):
    x = inputs(x_dtype, decode_dtype, batch)[0]
    return {"bs": to_device(np.ascontiguousarray(x[:, 1])),                          # (B, S): data level 1 = member 0
            "sb": to_device(np.ascontiguousarray(x[:, 1].T)),                        # (S, B)
            "g_bs": to_device(np.ascontiguousarray(x)),                              # (B, L, S)
            "g_sb": to_device(np.ascontiguousarray(x.transpose(1, 2, 0)))}           # (L, S, B)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    both_nan = np.isnan(got) & np.isnan(want) if got.dtype.kind == "f" else np.zeros(got.shape, bool)
    bad = np.argwhere((got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}")) & ~both_nan).tolist()
    assert not bad, f"{what}: {len(bad)} of {got.size} elements differ, first at {bad[:3]}"


class Call:
    """One grid point: the six `_pk` entries with raw status codes (no exception layer in between)."""

    def __init__(self, x_dtype, y_dtype, decode_dtype, skipna, batch):
        self.lib = _lib.load()
        self.g = geometry()
        self.x_dtype, self.y_dtype, self.batch = x_dtype, y_dtype, batch
        self.key = (x_dtype, decode_dtype, batch)
        x, cf, _ = inputs(*self.key)
        self.x = x
        self.cf = None if cf is None else cf._struct(x.dtype)
        self.enc = encode_rule(NP[y_dtype])._struct() if y_dtype in (I16, U16) else None
        self.flags = _lib.APPLY_MASKED | (_lib.APPLY_SKIPNA if skipna else 0)

    def _rules(self):
        return (None if self.cf is None else ctypes.byref(self.cf), None if self.enc is None else ctypes.byref(self.enc))

    def _y(self, shape):
        return np.full(shape, SENTINEL, dtype=np.uint8).view(NP[self.y_dtype]).reshape(shape[:-1] + (-1,))

    def _device(self, name, fn, x, mid, y_shape, rest):
        y = to_device(self._y(y_shape[:-1] + (y_shape[-1] * NP[self.y_dtype].itemsize,)))
        rc = getattr(self.lib, name)(fn, ctypes.c_void_p(x.ptr), self.x_dtype, *mid, ctypes.c_void_p(y.ptr), self.y_dtype,
                                     *rest, AREA_MIN, self.flags, None, *self._rules())
        return rc, self.lib.smm_last_error(), y.to_host()

    def _host(self, name, fn, x, mid, y_shape, rest, chunk):
        y = self._y(y_shape[:-1] + (y_shape[-1] * NP[self.y_dtype].itemsize,))
        rc = getattr(self.lib, name)(fn, x.ctypes.data_as(ctypes.c_void_p), self.x_dtype, *mid,
                                     y.ctypes.data_as(ctypes.c_void_p), self.y_dtype, *rest, AREA_MIN, self.flags, chunk,
                                     *self._rules())
        return rc, self.lib.smm_last_error(), y

    def run(self, entry, chunk=0):
        """(status, message, Y as (B, D) for the operator entries / (B, L, D) for the group entries)."""
        B, dev, op, grp = self.batch, device_inputs(*self.key), self.g["ops"][0].handle, self.g["grp"].handle
        lev, ml = LEV.ctypes.data_as(ctypes.c_void_p), MASKED_LEVELS.ctypes.data_as(ctypes.c_void_p)
        if entry == "smm_apply_pk":
            return self._device(entry, op, dev["bs"], (S,), (B, D), (D, B))
        if entry == "smm_apply_sb_pk":
            return self._device(entry, op, dev["sb"], (B,), (B, D), (D, B))
        if entry == "smm_apply_host_pk":
            return self._host(entry, op, np.ascontiguousarray(self.x[:, 1]), (S,), (B, D), (D, B), chunk)
        if entry == "smm_group_apply_pk":        # X (n_outer = B, L, n_inner = 1, S), Y transposed: (B, 1, L, D)
            return self._device(entry, grp, dev["g_bs"], (L * S, S, S), (B, L, D), (L * D, D, L * D, B, L, 1, lev, ml))
        if entry == "smm_group_apply_sb_pk":     # X (L, S, B), Y (B, L, D)
            return self._device(entry, grp, dev["g_sb"], (S * B, B), (B, L, D), (D, L * D, B, L, lev, ml))
        assert entry == "smm_group_apply_host_pk"
        return self._host(entry, grp, np.ascontiguousarray(self.x), (), (B, L, D), (B, L, 1, 1, lev, ml), chunk)


DEVICE_ENTRIES = ("smm_apply_pk", "smm_apply_sb_pk", "smm_group_apply_pk", "smm_group_apply_sb_pk")
HOST_ENTRIES = ("smm_apply_host_pk", "smm_group_apply_host_pk")


def three_chunks(batch):
    return -(-batch // 3)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("decode_dtype", [F32, F64], ids=lambda d: "dec_" + NAME[d])
@pytest.mark.parametrize("y_dtype", [F32, F64, I16, U16], ids=lambda d: "y_" + NAME[d])
@pytest.mark.parametrize("x_dtype", [F32, F64, I16, U16], ids=lambda d: "x_" + NAME[d])
def test_every_grid_point_through_the_six_pk_entries(hip, x_dtype, y_dtype, decode_dtype, skipna):
    refusal = STATUS[(x_dtype, y_dtype)]
    for batch in BATCHES:
        call = Call(x_dtype, y_dtype, decode_dtype, skipna, batch)
        runs = [(e, 0) for e in DEVICE_ENTRIES + HOST_ENTRIES] + [(e, three_chunks(batch)) for e in HOST_ENTRIES]
        if refusal is None:
            want_g = as_result(expectation(x_dtype, decode_dtype, skipna, batch), y_dtype)
            want_op = np.ascontiguousarray(want_g[:, 1])          # data level 1 is member 0, masked
            if y_dtype in (I16, U16):
                fill = encode_rule(NP[y_dtype]).fill_value
                assert 0.05 <= float((want_g != fill).mean()), "the expectation is all fill"
        for entry, chunk in runs:
            what = f"{entry} B={batch} chunk={chunk}"
            rc, msg, y = call.run(entry, chunk)
            if refusal is None:
                assert rc == _lib.SMM_OK, (what, rc, msg)
                same_bits(y, want_g if "group" in entry else want_op, what)
            else:
                assert rc == refusal[0] and refusal[1] in msg, (what, rc, msg)
                assert (y.view(np.uint8) == SENTINEL).all(), what + ": Y was written"


@pytest.mark.parametrize("entry", HOST_ENTRIES)
def test_injected_chunk_failure_leaves_the_pipeline_usable(hip, entry):
    """Chunk 1 of three fails: the error status comes back, and the next call on the same handle gives the right bits
    (the pipeline was drained, its buffers and streams are reusable)."""
    batch = 130
    call = Call(I16, I16, F32, False, batch)
    want = as_result(expectation(I16, F32, False, batch), I16)
    want = want if "group" in entry else np.ascontiguousarray(want[:, 1])
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        rc, msg, _ = call.run(entry, three_chunks(batch))
        assert rc == _lib.SMM_ERR_HIP and b"injected failure" in msg, (rc, msg)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    rc, msg, y = call.run(entry, three_chunks(batch))
    assert rc == _lib.SMM_OK, (rc, msg)
    same_bits(y, want, entry + " after the failure")
