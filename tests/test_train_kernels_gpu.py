"""K11's kernels one at a time (gmk_train_kernel_*: train_gemm_kernel in its direct and split-K forms, train_reduce_kernel, im2col3x3_kernel,
col2im3x3_kernel), on operands of the test's own, against tests/train_kernels_reference.py -- which tests/test_train_kernels_reference.py pins
on the CPU.  Bit for bit wherever arithmetic allows it (integer data, gathers, stated summation orders), inside the derived bound
gamma_(K+1) (sum |a| |b| + |bias|) elsewhere; the limit is 1 and is not tuned from the ratios recorded in profiles/train_parity.json.

Every operand lies in a buffer larger than its matrix: row padding and the zone behind it are NaN (an unguarded load would multiply it by the
other side's zero and show), the zone in front a finite sentinel.  Every output buffer is prefilled with a sentinel bit pattern and has guard
zones on both sides; after a run every float the descriptor does not name must still hold the sentinel's bits."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from gomokuai_amd import lib as G

import train_kernels_reference as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "train_parity.json")
GUARD = 96                                          # floats on either side of every buffer
FRONT = np.float32(12345.0)                         # before an operand's first element: in-range addressing never reaches it
GMK_ERR_ARG = -3


@pytest.fixture(autouse=True, scope="module")
def _device():
    G.init(0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _record(key, ratio):
    try:
        record = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        record[key] = {"worst_ratio": round(ratio, 4)}
        json.dump(record, open(PROFILE, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


class Buf:
    """A host array on the device between two guard zones.  ptr: the device address of its element 0."""

    def __init__(self, host, front, back, extra_front=0):
        self.n, self.at = host.size, GUARD + extra_front
        self.filled = np.concatenate([np.full(self.at, front, np.float32), np.asarray(host, np.float32), np.full(GUARD, back, np.float32)])
        self.t = torch.from_numpy(self.filled.copy()).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * self.at

    def read(self):
        return self.t.cpu().numpy()

    def refill(self):
        self.t.copy_(torch.from_numpy(self.filled))


def operand(host):
    return Buf(host, FRONT, np.nan)


def output(host, extra_front=0):
    return Buf(host, K.SENTINEL, K.SENTINEL, extra_front)


def upload(d):
    """the descriptor's host buffers -> {name: Buf} and the gmk_train_gemm_desc over them, every extent exactly the largest index + 1"""
    bufs = {name: operand(d[name]) for name in ("A", "B", "bias", "mask") if d[name] is not None}
    bufs.update({name: output(d[name], d["c_off"] if name == "C" else 0) for name in ("C", "C2", "part") if d[name] is not None})
    fields = {name: b.ptr for name, b in bufs.items()}                 # a buffer the form does not use stays NULL with extent 0
    for key in ("sam", "sak", "sbk", "sbn", "M", "N", "K", "kslab", "nz", "z0", "ldc", "cq", "cs", "nsplit", "ldc2", "relu", "ldm",
                "a_floats", "b_floats", "bias_floats", "mask_floats", "c_floats", "c2_floats", "part_floats"):
        fields[key] = d[key]
    return bufs, G.train_gemm_desc(**fields)


def run_gemm(d):
    """-> (bufs, desc, {"C", "C2", "part": the whole device buffer, guards included, after the call})"""
    bufs, desc = upload(d)
    G.train_kernel_gemm(desc)
    torch.cuda.synchronize()
    return bufs, desc, {name: bufs[name].read() for name in ("C", "C2", "part") if name in bufs}


def expected_buffers(d, bufs, values, dtype=np.float32):
    """what the whole device buffers must hold: the prefill, and `values` (the shape of gemm_logical) where the descriptor stores them"""
    out, written = K.scatter(d, values)
    full, where = {}, {}
    for name in ("C", "C2", "part"):
        if d[name] is None:
            continue
        b = bufs[name]
        full[name] = b.filled.astype(dtype)
        full[name][b.at:b.at + b.n] = out[name].astype(dtype)
        where[name] = np.zeros(b.filled.size, bool)
        where[name][b.at:b.at + b.n] = written[name]
    return full, where


def check_untouched(d, bufs, got, where):
    for name, g in got.items():
        stale = _bits(g)[~where[name]] != _bits(bufs[name].filled)[~where[name]]
        assert not stale.any(), "%s: %s has %d floats written outside the descriptor's map, first at %d (element 0 is at %d)" % (
            d["name"], name, int(stale.sum()), int(np.nonzero(~where[name])[0][np.argmax(stale)]), bufs[name].at)
    for name, b in bufs.items():
        if name not in got:
            assert np.array_equal(_bits(b.read()), _bits(b.filled)), "%s: operand %s changed" % (d["name"], name)


def check_exact(d):
    bufs, _, got = run_gemm(d)
    want, where = expected_buffers(d, bufs, K.gemm_logical(d))
    for name, g in got.items():
        assert not np.isnan(g).any(), "%s: NaN in %s: an unguarded operand load" % (d["name"], name)
        diff = np.nonzero(_bits(g) != _bits(want[name]))[0]
        assert diff.size == 0, "%s: %s differs at %d floats, first at %d (got %r, want %r; element 0 is at %d)" % (
            d["name"], name, diff.size, diff[0], g[diff[0]], want[name][diff[0]], bufs[name].at)
    check_untouched(d, bufs, got, where)
    return bufs, got


def check_bound(d, record=None):
    bufs, _, got = run_gemm(d)
    _, where = expected_buffers(d, bufs, K.gemm_logical(d))
    check_untouched(d, bufs, got, where)
    inner = {name: g[bufs[name].at:bufs[name].at + bufs[name].n] for name, g in got.items()}
    logical = K.gather_logical(d, inner)
    assert not np.isnan(logical).any(), "%s: NaN in the result: an unguarded operand load" % d["name"]
    ratio = K.worst_ratio(d, logical)
    print("%s: worst |got - float64| / bound = %.4f" % (d["name"], ratio))
    if record:
        _record(record, ratio)
    assert ratio <= 1.0, (d["name"], ratio)
    return bufs, inner


# ---------------------------------------------------------------------------------------------------------------- exact
def _params(cases):
    return pytest.mark.parametrize("case", cases, ids=[c["name"] for c in cases])


@_params(K.shape_cases())
def test_gemm_exact_across_tile_and_k_edges(case):
    check_exact(K.materialize(case, "int"))


@_params(K.layout_cases())
def test_gemm_exact_in_every_layout(case):
    check_exact(K.materialize(case, "int"))


@_params(K.split_cases())
def test_gemm_exact_split_k(case):
    """raw partial sums in slabs z0 .. z0 + nz - 1; the slabs below z0 keep the sentinel, and bias / ReLU / mask change nothing"""
    check_exact(K.materialize(case, "int"))


@_params(K.epilogue_cases())
def test_gemm_exact_epilogue(case):
    check_exact(K.materialize(case, "int"))


@_params(K.trainer_cases())
def test_gemm_exact_on_the_trainers_own_descriptors(case):
    """every GemmArgs of run_forward, run_backward and column_sums at n = 9, over integer data"""
    check_exact(K.materialize(case, "int"))


@_params(K.reduce_cases())
def test_reduce_is_the_float32_sum_in_slab_order(case):
    """real-valued partials from the device's own split-K GEMM (so the order matters), then train_reduce_kernel, bit for bit"""
    d = K.materialize(case, "real")
    bufs, part = check_bound(d)
    mn, nz = d["M"] * d["N"], d["nz"]
    out = output(np.full(mn, K.SENTINEL, np.float32))
    G.train_kernel_reduce(bufs["part"].ptr, nz, mn, out.ptr)
    torch.cuda.synchronize()
    want = out.filled.copy()
    want[out.at:out.at + mn] = K.reduce_ref(part["part"], nz, mn)
    got = out.read()
    assert np.array_equal(_bits(got), _bits(want)), (d["name"], int((_bits(got) != _bits(want)).sum()))
    assert np.array_equal(_bits(bufs["part"].read()[bufs["part"].at:][:nz * mn]), _bits(part["part"]))
    whole = dict(d, split=False, nz=1, kslab=d["K"])                  # the two stages together are one sum of K products
    assert (np.abs(got[out.at:out.at + mn].astype(np.float64) - K.gemm_logical(d).sum(0).reshape(-1)) <= K.gemm_bound(whole).reshape(-1)).all()


# ---------------------------------------------------------------------------------------------------------------- rounded
@_params(K.rounded_cases())
def test_gemm_real_valued_inside_the_derived_bound(case):
    check_bound(K.materialize(case, "real"), record="kernel-" + case["name"])


# ---------------------------------------------------------------------------------------------------------------- properties
PROPERTY_CASES = [K.make_case("prop-257x31x450", 257, 31, 450), K.make_case("prop-257x63x33-am", 257, 63, 33, a="m", b="n", pad=1),
                  K.make_case("prop-257x129x17-bias", 257, 129, 17, bias=True, relu=1),
                  K.make_case("prop-129x65x450-split", 129, 65, 450, a="m", b="n", split=True, kslab=17, z0=1)]


@_params(PROPERTY_CASES)
def test_repeats_give_the_same_bits(case):
    d = K.materialize(case, "real")
    bufs, desc, first = run_gemm(d)
    for name in first:
        bufs[name].refill()
    G.train_kernel_gemm(desc)
    torch.cuda.synchronize()
    for name, g in first.items():
        assert np.array_equal(_bits(bufs[name].read()), _bits(g)), (case["name"], name)
        assert not np.isnan(g).any()


@_params(PROPERTY_CASES[:3])
def test_rows_equal_the_one_row_gemm(case):
    """rows 0, 31, 32, 127, 128, M - 1 equal the GEMM of that row alone (M = 1, A starting at the row), whatever the other rows of A hold:
    the k order of a row does not depend on M or on the row's place in its tile"""
    d = K.materialize(case, "real")
    M, N = d["M"], d["N"]
    rows = (0, 31, 32, 127, 128, M - 1)
    _, inner = check_bound(d)
    where = K.index_out(d)[1]                                          # [M][N]: where C(m, n) lies
    whole = inner["C"][where]
    poisoned = dict(d, A=d["A"].copy())
    ia = K.index_a(d)
    poisoned["A"][np.setdiff1d(ia, ia[list(rows)])] = np.nan
    for A, label in ((d["A"], "finite"), (poisoned["A"], "NaN")):
        for r in rows:
            one = dict(d, name="%s-row%d" % (d["name"], r), M=1, A=A[r * d["sam"]:][:(d["K"] - 1) * d["sak"] + 1])
            one["a_floats"], one["c_floats"] = one["A"].size, d["row_extent"]
            one["C"] = np.full(d["row_extent"], K.SENTINEL, np.float32)
            if label == "NaN":
                assert not np.isnan(one["A"][K.index_a(one)]).any()
            bufs, _, got = run_gemm(one)
            alone = got["C"][bufs["C"].at:][:N]
            assert np.array_equal(_bits(alone), _bits(whole[r])), (case["name"], r, label)
    # and the full GEMM over the poisoned A: the chosen rows are what they were
    bufs, _, got = run_gemm(poisoned)
    again = got["C"][bufs["C"].at:][where]
    for r in rows:
        assert np.array_equal(_bits(again[r]), _bits(whole[r])), (case["name"], r, "within NaN rows")


def test_columns_against_the_column_alone_is_printed():
    """N = 33 (the 128 x 64 variant) against each column alone (N = 1, the 128 x 32 variant): DESIGN.md promises an order that depends on the
    shapes only, not that two variants agree -- so this reports, and asserts only the bound on both sides."""
    d = K.materialize(K.make_case("prop-columns-129x33x450", 129, 33, 450), "real")
    _, inner = check_bound(d)
    whole = inner["C"].reshape(129, 33)
    differ = 0
    for n in (0, 31, 32):
        one = dict(d, name="%s-col%d" % (d["name"], n), N=1, B=d["B"][n * d["sbn"]:][:d["K"]], ldc=1, row_extent=1)
        one["b_floats"], one["c_floats"], one["C"] = one["B"].size, 129, np.full(129, K.SENTINEL, np.float32)
        _, alone = check_bound(one)
        differ += int((_bits(alone["C"]) != _bits(whole[:, n])).sum())
    print("column independence across variants: %d of %d floats differ" % (differ, 3 * 129))


# ---------------------------------------------------------------------------------------------------------------- im2col, col2im
CONV = [(C_, npos) for C_ in K.CONV_C for npos in K.CONV_NPOS]


@pytest.mark.parametrize("C_,npos", CONV)
@pytest.mark.parametrize("layout", ("planes", "channels-last", "channels-last-padded"))
def test_im2col_is_the_stated_gather(C_, npos, layout):
    sb, sp, sc = {"planes": (C_ * 225, 1, 225), "channels-last": (C_ * 225, C_, 1), "channels-last-padded": (225 * (C_ + 1) + 7, C_ + 1, 1)}[layout]
    extent = (npos - 1) * sb + 224 * sp + (C_ - 1) * sc + 1
    rng = np.random.default_rng([C_, npos, len(layout)])
    host = np.full(extent, np.nan, np.float32)
    used = np.unique(np.arange(npos)[:, None, None] * sb + np.arange(225)[None, :, None] * sp + np.arange(C_)[None, None, :] * sc)
    host[used] = rng.standard_normal(used.size).astype(np.float32)
    assert (layout == "channels-last-padded") == bool(np.isnan(host).any())
    src, col = operand(host), output(np.full(npos * 225 * 9 * C_, K.SENTINEL, np.float32))
    G.train_kernel_im2col(src.ptr, extent, sb, sp, sc, C_, npos, col.ptr)
    torch.cuda.synchronize()
    want = col.filled.copy()
    ref = K.im2col_ref(host, sb, sp, sc, C_, npos)
    want[col.at:col.at + col.n] = ref.reshape(-1)
    got = col.read()
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want))
    # 'same' padding: exact +0.0 at the four borders and corners, for every channel
    g = got[col.at:col.at + col.n].reshape(npos, 15, 15, C_, 3, 3)
    for edge in (g[:, 0, :, :, 0, :], g[:, 14, :, :, 2, :], g[:, :, 0, :, :, 0], g[:, :, 14, :, :, 2]):
        assert not _bits(edge).any()
    assert np.array_equal(_bits(src.read()), _bits(src.filled))


MASKS = np.array([1.0, 1e-30, 7.5, 0.0, -0.0, -2.0, np.nan], np.float32)


@pytest.mark.parametrize("C_,npos", CONV)
def test_col2im_is_the_gather_in_tap_order(C_, npos):
    rng = np.random.default_rng([C_, npos, 77])
    rows = npos * 225
    dcol = (rng.standard_normal((rows, 9 * C_)) * np.exp2(rng.integers(-8, 9, (rows, 9 * C_)))).astype(np.float32)
    mask = MASKS[rng.choice(MASKS.size, rows * C_, p=[0.3, 0.2, 0.2, 0.075, 0.075, 0.075, 0.075])]
    mask[:MASKS.size] = MASKS                                          # every kind at least once
    ref32, mag = K.col2im_ref(dcol, C_, npos, mask, np.float32)
    ref64, _ = K.col2im_ref(dcol, C_, npos, mask, np.float64)
    src, msk, out = operand(dcol.reshape(-1)), operand(mask), output(np.full(rows * C_, K.SENTINEL, np.float32))
    G.train_kernel_col2im(src.ptr, C_, npos, msk.ptr, out.ptr)
    torch.cuda.synchronize()
    want = out.filled.copy()
    want[out.at:out.at + out.n] = ref32.reshape(-1)
    got = out.read()
    assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want))
    inner = got[out.at:out.at + out.n].astype(np.float64)
    assert (np.abs(inner - ref64.reshape(-1)) <= 9 * K.U * mag.reshape(-1)).all()
    with np.errstate(invalid="ignore"):
        keep = mask > 0
    assert (inner[~keep] == 0).all() and (inner[keep] != 0).any()
    # NaN in one row of the columns (9 C numbers): it shows in the outputs that read them and are kept, nowhere else
    row = rows // 2 + 16
    dcol[row] = np.nan
    ref32, _ = K.col2im_ref(dcol, C_, npos, mask, np.float32)
    expect_nan = np.isnan(ref32.reshape(-1))
    assert expect_nan.sum() <= 9 * C_
    src2 = operand(dcol.reshape(-1))
    out.refill()
    G.train_kernel_col2im(src2.ptr, C_, npos, msk.ptr, out.ptr)
    torch.cuda.synchronize()
    got = out.read()
    inner = got[out.at:out.at + out.n]
    assert np.array_equal(np.isnan(inner), expect_nan)
    assert np.array_equal(_bits(inner[~expect_nan]), _bits(ref32.reshape(-1)[~expect_nan]))
    assert np.array_equal(_bits(got[:out.at]), _bits(out.filled[:out.at])) and np.array_equal(_bits(got[out.at + out.n:]), _bits(out.filled[out.at + out.n:]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _snapshot(bufs):
    return {name: _bits(b.read()).copy() for name, b in bufs.items()}


def _refused(call, field, bufs, before):
    rc = call()
    assert rc == GMK_ERR_ARG, (field, rc)
    named = re.search(rb"refused, (?:field|argument) (\w+)", G.load().gmk_last_error())
    assert named and named.group(1) == field.encode(), (field, G.load().gmk_last_error())
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert np.array_equal(_bits(b.read()), before[name]), (field, name)


def test_gemm_refuses_what_does_not_fit_before_launch():
    """Every descriptor fault of include/gomoku_hip.h: GMK_ERR_ARG with the field named, no bit of any buffer changed, and the next valid call
    on the stream is right.  (tools/train_host_check.cpp walks the same check, gemm_fits, without a device.)"""
    L = G.load()
    direct = K.materialize(K.make_case("refuse-direct", 33, 6, 17, bias=True, relu=1, mask=True, nsplit=4, ldc=4, ldc2=2, pad=0), "int")
    grouped = K.materialize(K.make_case("refuse-grouped", 9, 10, 15, cq=3, cs=5, pad=2), "int")
    split = K.materialize(K.make_case("refuse-split", 33, 6, 17, split=True, kslab=7, z0=1), "int")
    for d, faults in (
        (direct, [("A", dict(A=None)), ("A", dict(A=+2)), ("B", dict(B=None)), ("B", dict(B=+2)), ("C", dict(C=None)), ("C", dict(C=+2)),
                  ("C2", dict(C2=None)), ("C2", dict(C2=+2)), ("bias", dict(bias=+2)), ("mask", dict(mask=+2)),
                  ("sam", dict(sam=-1)), ("sak", dict(sak=-1)), ("sbk", dict(sbk=-1)), ("sbn", dict(sbn=-1)), ("ldm", dict(ldm=-1)),
                  ("M", dict(M=0)), ("N", dict(N=0)), ("K", dict(K=0)), ("M", dict(M=-1)),
                  ("kslab", dict(kslab=0)), ("nz", dict(kslab=16)), ("nz", dict(nz=2)), ("nz", dict(nz=2, kslab=9)), ("nz", dict(nz=0)),
                  ("a_floats", dict(a_floats=-1)), ("b_floats", dict(b_floats=-1)), ("c_floats", dict(c_floats=-1)), ("c2_floats", dict(c2_floats=-1)),
                  ("mask_floats", dict(mask_floats=-1)), ("bias", dict(bias_floats=-1)),
                  ("ldc", dict(ldc=3)), ("ldc2", dict(ldc2=1)), ("ldc", dict(nsplit=6)), ("nsplit", dict(nsplit=-1)), ("cq", dict(cq=0)), ("relu", dict(relu=2))]),
        (grouped, [("cs", dict(cs=2)), ("cs", dict(cs=-5)), ("ldc", dict(ldc=15)), ("c_floats", dict(c_floats=-1)), ("C2", dict(nsplit=7))]),
        (split, [("part", dict(part=+2)), ("nz", dict(nz=2)), ("nz", dict(nz=4)), ("nz", dict(kslab=1 << 30, nz=2)), ("z0", dict(z0=-1)),
                 ("part_floats", dict(part_floats=-1)), ("part_floats", dict(z0=2)), ("kslab", dict(kslab=0)), ("a_floats", dict(a_floats=-1))]),
    ):
        bufs, desc = upload(d)
        before = _snapshot(bufs)
        for field, change in faults:
            bad = G.TrainGemmDesc.from_buffer_copy(desc)
            for key, value in change.items():
                if key in bufs or key in ("A", "B", "C", "C2", "bias", "mask", "part"):
                    setattr(bad, key, None if value is None else getattr(desc, key) + value)          # NULL, or two bytes off alignment
                elif key.endswith("_floats"):
                    setattr(bad, key, getattr(desc, key) + value)                                       # one float short
                else:
                    setattr(bad, key, value)
            _refused(lambda: L.gmk_train_kernel_gemm(C.byref(bad), None), field, bufs, before)
        assert L.gmk_train_kernel_gemm(None, None) == GMK_ERR_ARG
        G.train_kernel_gemm(desc)                                                                      # the same stream, a valid descriptor
        torch.cuda.synchronize()
        got = {name: bufs[name].read() for name in ("C", "C2", "part") if name in bufs}
        want, _ = expected_buffers(d, bufs, K.gemm_logical(d))
        for name, g in got.items():
            assert np.array_equal(_bits(g), _bits(want[name])), (d["name"], name)


def test_reduce_im2col_col2im_refuse_what_does_not_fit():
    L = G.load()
    host = np.arange(3 * 1125, dtype=np.float32)
    src, col, out = operand(host), output(np.full(3 * 225 * 45, K.SENTINEL, np.float32)), output(np.full(3 * 1125, K.SENTINEL, np.float32))
    bufs = {"src": src, "col": col, "out": out}
    before = _snapshot(bufs)

    def im2col(**kw):
        a = dict(dict(inp=src.ptr, in_floats=3 * 1125, sb=1125, sp=5, sc=1, C=5, npos=3, col=col.ptr), **kw)
        return lambda: L.gmk_train_kernel_im2col(a["inp"], a["in_floats"], a["sb"], a["sp"], a["sc"], a["C"], a["npos"], a["col"], None)

    for field, kw in (("in_floats", dict(in_floats=3 * 1125 - 1)), ("in", dict(inp=None)), ("in", dict(inp=src.ptr + 2)), ("col", dict(col=None)),
                      ("sb", dict(sb=-1)), ("sp", dict(sp=-5)), ("sc", dict(sc=-1)), ("C", dict(C=0)), ("npos", dict(npos=0)), ("npos", dict(npos=1 << 30)),
                      ("in_floats", dict(sp=1, sc=225, in_floats=3 * 1125 - 1))):
        _refused(im2col(**kw), field, bufs, before)
    for field, call in (("dcol", lambda: L.gmk_train_kernel_col2im(None, 5, 3, src.ptr, out.ptr, None)),
                        ("mask", lambda: L.gmk_train_kernel_col2im(col.ptr, 5, 3, None, out.ptr, None)),
                        ("out", lambda: L.gmk_train_kernel_col2im(col.ptr, 5, 3, src.ptr, out.ptr + 2, None)),
                        ("C", lambda: L.gmk_train_kernel_col2im(col.ptr, 0, 3, src.ptr, out.ptr, None)),
                        ("npos", lambda: L.gmk_train_kernel_col2im(col.ptr, 5, -1, src.ptr, out.ptr, None)),
                        ("part", lambda: L.gmk_train_kernel_reduce(None, 1, 5, out.ptr, None)),
                        ("out", lambda: L.gmk_train_kernel_reduce(src.ptr, 1, 5, None, None)),
                        ("nz", lambda: L.gmk_train_kernel_reduce(src.ptr, 0, 5, out.ptr, None)),
                        ("mn", lambda: L.gmk_train_kernel_reduce(src.ptr, 1, 0, out.ptr, None)),
                        ("mn", lambda: L.gmk_train_kernel_reduce(src.ptr, 1, 1 << 31, out.ptr, None))):
        _refused(call, field, bufs, before)
    G.train_kernel_im2col(src.ptr, 3 * 1125, 1125, 5, 1, 5, 3, col.ptr)
    G.train_kernel_reduce(src.ptr, 3, 1125, out.ptr)
    torch.cuda.synchronize()
    assert np.array_equal(col.read()[col.at:col.at + col.n], K.im2col_ref(host, 1125, 5, 1, 5, 3).reshape(-1))
    assert np.array_equal(out.read()[out.at:out.at + 1125], K.reduce_ref(host, 3, 1125))
