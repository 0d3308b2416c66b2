"""The float64 restatement of K11's kernels (tests/train_kernels_reference.py) and its derived bound earn their trust on the CPU, before the
kernels are held to them in tests/test_train_kernels_gpu.py: correct float32 products stay inside the bound, planted faults leave it (or
fail the exact comparison) on every case of their class, and the case tables hold the edges they claim."""
import os
import re

import numpy as np
import pytest
import torch

import train_kernels_reference as K

REAL = [K.materialize(c, "real") for c in K.rounded_cases()]
INT = [K.materialize(c, "int") for c in K.exact_cases() + K.trainer_cases()]
ids = lambda cases: [d["name"] for d in cases]


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _faulty(d, fault):
    """gemm_logical(d) in float64 with one fault planted"""
    a, b = K.operands(d)
    ranges = K.slabs(d)
    if fault == "drop_last_k":
        ranges = ranges[:-1] + ([(ranges[-1][0], ranges[-1][1] - 1)])
    elif fault == "kend_off_by_one":                    # one slab (the middle one, if there is one) stops a k early
        z = len(ranges) // 2
        ranges = ranges[:z] + [(ranges[z][0], ranges[z][1] - 1)] + ranges[z + 1:]
    elif fault == "swap_b_columns":
        b = b.copy()
        b[:, [0, d["N"] - 1]] = b[:, [d["N"] - 1, 0]]
    elif fault == "bf16_operands":
        a, b = _bf16(a), _bf16(b)
    sums = [a[:, k0:k1] @ b[k0:k1] + 0.0 for k0, k1 in ranges]
    if d["split"]:
        return np.stack(sums)
    s = sum(sums)
    if fault == "relu_before_bias":                     # the wrong order: ReLU, then the bias; the mask stays last
        assert d["relu"] and d["bias"] is not None
        return K.epilogue(dict(d, bias=None, relu=0), np.maximum(s, 0) + d["bias"].astype(np.float64)[None, :]) + 0.0
    return K.epilogue(d, s) + 0.0


# ---------------------------------------------------------------------------------------------------------------- the yardstick cuts both ways
@pytest.mark.parametrize("d", REAL, ids=ids(REAL))
def test_float32_products_stay_inside_the_bound(d):
    assert K.worst_ratio(d, K.gemm_logical(d)) == 0.0
    for name, mm in (("numpy", None), ("torch", lambda x, y: torch.mm(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y))).numpy())):
        got = K.gemm_logical(d, matmul=mm, dtype=np.float32)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert K.worst_ratio(d, got) <= 1.0, (name, K.worst_ratio(d, got))


@pytest.mark.parametrize("fault", ("drop_last_k", "swap_b_columns", "bf16_operands"))
@pytest.mark.parametrize("d", REAL, ids=ids(REAL))
def test_planted_faults_leave_the_bound(d, fault):
    assert K.worst_ratio(d, _faulty(d, fault)) > 1.0
    assert K.worst_ratio(d, _faulty(d, None)) == 0.0


@pytest.mark.parametrize("d", INT, ids=ids(INT))
def test_off_by_one_kend_fails_the_exact_comparison(d):
    want = K.gemm_logical(d)
    assert np.array_equal(_faulty(d, None), want)
    assert not np.array_equal(_faulty(d, "kend_off_by_one"), want)


RELU_BIAS = [d for d in INT if d["relu"] and d["bias"] is not None and not d["split"]]


@pytest.mark.parametrize("d", RELU_BIAS, ids=ids(RELU_BIAS))
def test_relu_before_bias_fails_the_exact_comparison(d):
    assert not np.array_equal(_faulty(d, "relu_before_bias"), K.gemm_logical(d))


def test_integer_sums_are_exact_in_float32_in_any_order():
    """what makes the exact cases exact: float32 products in numpy's order, and in reversed k order, give float64's bits"""
    for d in INT[::7]:
        want = K.gemm_logical(d)
        assert np.abs(want).max() < 2 ** 24 and np.array_equal(want, np.round(want))
        assert np.array_equal(K.gemm_logical(d, dtype=np.float32).astype(np.float64), want)
        back = K.gemm_logical(d, matmul=lambda x, y: x[:, ::-1] @ y[::-1], dtype=np.float32)
        assert np.array_equal(back.astype(np.float64), want)


def test_gemm_ref_writes_what_the_descriptor_says_and_nothing_else():
    for d in INT:
        out, written = K.scatter(d, K.gemm_logical(d))
        for name in ("C", "C2", "part"):
            if d[name] is None:
                assert out[name] is None
                continue
            assert (out[name][~written[name]] == K.SENTINEL).all() and not (out[name][written[name]] == K.SENTINEL).any()
        assert np.array_equal(K.gather_logical(d, out), K.gemm_logical(d))
        count = sum(int(w.sum()) for w in written.values() if w is not None)
        assert count == d["M"] * d["N"] * (d["nz"] if d["split"] else 1)
    # by hand: 2 x 3 x 2, bias, ReLU, mask, the columns of C three floats apart, column 2 on in C2
    c = K.make_case("hand", 2, 3, 2, bias=True, relu=1, mask=True, cq=1, cs=3, nsplit=2, ldc=5, ldc2=2)
    d = K.materialize(c)
    d["A"][:] = [1, 2, 3, -4]
    d["B"][:] = [1, 0, -1, 1, 2, 2]                     # B[n][k]: columns (1, 0), (-1, 1), (2, 2)
    d["bias"][:] = [-2, 1, 0]
    d["mask"][:] = [1, -0.0, 5, 2, 3, np.nan]
    ref = K.gemm_ref(d)
    s = K.SENTINEL
    # sums [[1, 1, 6], [3, -7, -2]] + bias -> [[-1, 2, 6], [1, -6, -2]] -> ReLU [[0, 2, 6], [1, 0, 0]] -> mask [[0, 0, 6], [1, 0, 0]]
    assert ref["C"].tolist() == [0, s, s, 0, s, 1, s, s, 0] and ref["C2"].tolist() == [6, s, 0] and ref["part"] is None


def test_bound_is_the_stated_formula():
    d = K.materialize(K.make_case("b", 1, 1, 3, bias=True), "real")
    d["A"][:], d["B"][:], d["bias"][:] = [1, -2, 4], [0.5, 3, -1], [-8]
    g = 4 * 2.0 ** -24 / (1 - 4 * 2.0 ** -24)
    assert K.gemm_bound(d).tolist() == [[g * (0.5 + 6 + 4 + 8) + 2.0 ** -126]]
    assert K.reduce_ref(np.array([1, 2 ** 24, 1, -2 ** 24], np.float32), 4, 1).tolist() == [0.0]          # ((0 + 1) + 2^24) + 1 - 2^24 in float32
    assert K.reduce_ref(np.arange(6, dtype=np.float32), 2, 3).tolist() == [3, 5, 7]


# ---------------------------------------------------------------------------------------------------------------- im2col and col2im
def test_im2col_then_gemm_is_conv2d():
    """column cin * 9 + tap is [cout][cin][3][3] flattened"""
    rng = np.random.default_rng(5)
    for C, cout, npos in ((5, 7, 2), (6, 32, 1)):
        x, w, bias = rng.standard_normal((npos, C, 15, 15)), rng.standard_normal((cout, C, 3, 3)), rng.standard_normal(cout)
        want = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias), padding=1).clamp_min(0).numpy()
        for layout in ("planes", "channels-last"):
            buf, (sb, sp, sc) = (x.reshape(-1), (C * 225, 1, 225)) if layout == "planes" else (x.transpose(0, 2, 3, 1).reshape(-1), (C * 225, C, 1))
            col = K.im2col_ref(buf, sb, sp, sc, C, npos)
            d = K.make_case("conv", npos * 225, cout, 9 * C, bias=True, relu=1)
            d.update(A=col.reshape(-1), B=w.reshape(-1), bias=bias, mask=None, C=np.zeros(npos * 225 * cout), C2=None, part=None)
            got = K.gemm_ref(d)["C"].reshape(npos, 15, 15, cout).transpose(0, 3, 1, 2)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_col2im_is_the_adjoint_of_im2col():
    rng = np.random.default_rng(6)
    for C in K.CONV_C:
        for npos in K.CONV_NPOS:
            x, y = rng.standard_normal(npos * 225 * C), rng.standard_normal((npos * 225, 9 * C))
            col = K.im2col_ref(x, 225 * C, C, 1, C, npos)
            back, mag = K.col2im_ref(y, C, npos, np.ones(npos * 225 * C), np.float64)
            lhs, rhs = (col * y).sum(), (x * back.reshape(-1)).sum()
            assert abs(lhs - rhs) <= 1e-12 * (np.abs(col * y).sum()), (C, npos)
            assert mag.shape == back.shape and (mag >= np.abs(back) - 1e-12).all()
    # the corner pixel appears in four columns, an inner pixel in nine; the mask keeps only > 0
    ones = np.ones((225, 9))
    back, _ = K.col2im_ref(ones, 1, 1, np.ones(225))
    assert back[0, 0] == 4 and back[14, 0] == 4 and back[7, 0] == 6 and back[16, 0] == 9 and back.dtype == np.float32
    mask = np.ones(225, np.float32)
    mask[:4] = [0.0, -0.0, -1.0, np.nan]
    assert K.col2im_ref(ones, 1, 1, mask)[0][:5, 0].tolist() == [0, 0, 0, 0, 6]


def test_im2col_pads_with_exact_zeros():
    x = np.arange(1, 226, dtype=np.float32)
    col = K.im2col_ref(x, 225, 1, 225, 1, 1)
    assert col[0].tolist() == [0, 0, 0, 0, 1, 2, 0, 16, 17] and col[224].tolist() == [209, 210, 0, 224, 225, 0, 0, 0, 0]
    assert col[14].tolist() == [0, 0, 0, 14, 15, 0, 29, 30, 0] and col[210].tolist() == [0, 196, 197, 0, 211, 212, 0, 0, 0]
    assert (col == 0).sum() == 4 * 15 * 3 - 4 and col[16 * 7].min() > 0


# ---------------------------------------------------------------------------------------------------------------- the tables
def test_case_tables_hold_the_edges_they_claim():
    shapes = K.shape_cases()
    assert 35 <= len(shapes) <= 45 and len({c["name"] for c in K.exact_cases() + K.trainer_cases() + K.rounded_cases()}) == len(K.exact_cases() + K.trainer_cases() + K.rounded_cases())
    assert {c["M"] for c in shapes} == set(K.M_LIST) and {c["N"] for c in shapes} == set(K.N_LIST) and {c["K"] for c in shapes} == set(K.K_LIST)
    combos = {(K.variant(c["N"]), c["M"] % 32, c["K"] % 16) for c in shapes}
    assert {(v, m, k) for v in range(3) for m in (0, 1, 31) for k in (0, 1, 15)} <= combos
    assert [K.variant(n) for n in (32, 33, 64, 65)] == [0, 1, 1, 2] and {m % 32 for m in K.M_LIST} == {0, 1, 31}
    lay = K.layout_cases()
    for v in range(3):
        mine = [c for c in lay if K.variant(c["N"]) == v]
        for pad in (0, 3):
            seen = {(c["sak"] == 1, c["sbk"] == 1) for c in mine if c["pad"] == pad and c["K"] > 1 and c["a"] != "0" and c["b"] != "0n"}
            assert seen == {(True, True), (True, False), (False, True), (False, False)}
            assert any(c["sam"] == 0 and c["sak"] == 0 and c["M"] == 1 for c in mine if c["pad"] == pad)
            assert any(c["sbn"] == 0 and c["N"] > 1 for c in mine if c["pad"] == pad)
            assert any(c["K"] == 1 and c["sak"] == 1 and c["sbk"] == 1 for c in mine if c["pad"] == pad)
    assert any(c["sbn"] == 0 and c["N"] == 1 for c in lay)
    pads = [K.materialize(c) for c in lay if c["pad"]]
    assert all(np.isnan(d["A"]).any() or d["a"] == "0" for d in pads) and all(np.isnan(d["B"]).any() or d["b"] == "0n" for d in pads)
    split = K.split_cases()
    assert {c["kslab"] for c in split} >= {1, 2, 7, 16, 17, 1800} and {c["z0"] for c in split} >= {0, 3}
    assert all(c["K"] % c["kslab"] != 0 or c["kslab"] == 1 for c in split) and all(c["nz"] == -(-c["K"] // c["kslab"]) for c in split)
    assert any(c["K"] == 3607 and c["nz"] == 3 for c in split) and {K.variant(c["N"]) for c in split if c["kslab"] == 1800} == {0, 1, 2}
    assert sum(1 for c in split if c["has_bias"] and c["relu"] and c["has_mask"]) == 3
    red = K.reduce_cases()
    assert {c["M"] * c["N"] for c in red} == {1, 255, 256, 257, 768} and {c["nz"] for c in red} == {1, 2, 33} and len(red) == 15
    epi = K.epilogue_cases()
    assert {(c["nsplit"], c["ldc"], c["ldc2"]) for c in epi if "nsplit" in c["name"]} == {(0, 4, 6), (4, 4, 2), (6, 6, 2)}
    assert {(c["cq"], c["cs"], c["N"], c["c_off"]) for c in epi if c["cq"] < c["N"] and c["nsplit"] == K.NONE} == {(4, 6, 900, 0), (2, 6, 450, 4), (3, 5, 10, 0)}
    assert any(c["has_bias"] and c["relu"] and c["has_mask"] and c["cq"] < c["N"] and c["nsplit"] < c["N"] for c in epi)
    for d in (K.materialize(c) for c in epi):
        if d["bias"] is not None:
            assert (d["bias"] < 0).any() and (d["bias"] > 0).any()
        if d["relu"] and d["bias"] is not None and d["mask"] is None:
            pre = K.gemm_logical(dict(d, relu=0))
            assert (pre < 0).any() and (pre > 0).any()                   # ReLU zeroes some results and keeps others
        if d["mask"] is not None:
            m = d["mask"][K.index_mask(d)]
            assert (m > 0).any() and (m == 0).any() and np.signbit(m[m == 0]).any() and (m < 0).any() and np.isnan(m).any()
    real = K.rounded_cases()
    assert 9 <= len(real) <= 12 and any(c["K"] == 17 for c in real) and any(c["K"] == 3607 and c["nz"] == 3 for c in real)
    assert any(c["has_bias"] and not c["split"] for c in real) and any(c["has_mask"] for c in real)
    for d in REAL:
        for buf in (d["A"], d["B"]):
            v = np.abs(buf[~np.isnan(buf)])
            assert (v == 0).any() and v[v > 0].min() >= 2.0 ** -20 and v.max() <= 2.0 ** 20 and np.log2(v.max() / v[v > 0].min()) > 30


def test_trainer_table_matches_the_trainers_constants():
    """The table restates train_kernel.hip's launches at n = 9; the sizes it assumes are train_host.h's."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gomokuai_amd", "csrc", "train_host.h")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (kPix|kSlabPos|kKSlabPos) = (\d+);", src)}
    assert const == {"kPix": 225, "kSlabPos": 32, "kKSlabPos": 8} and K.PIX == const["kPix"]
    sizes = [eval(e) for e in re.search(r"kSizes\[kTensors\] = \{([^}]*)\}", src).group(1).split(",")]
    n = 9
    assert n <= const["kSlabPos"]                                        # one position slab
    rows, ks = n * const["kPix"], const["kKSlabPos"] * const["kPix"]
    table = {c["name"][len("trainer-"):]: c for c in K.trainer_cases(n)}
    assert len(table) == 25 and rows == 2025
    weights = {"conv1": 0, "conv2": 2, "conv3": 4, "logits": 10, "hidden": 12}
    for name, t in weights.items():                                      # forward: N x K is the weight tensor, N its bias
        c = table[name]
        assert c["N"] * c["K"] == sizes[t] and c["N"] == sizes[t + 1] and c["has_bias"] and c["M"] == (n if t >= 10 else rows)
    assert table["heads"]["N"] * table["heads"]["K"] == sizes[6] + sizes[7] and (table["heads"]["nsplit"], table["heads"]["N"]) == (sizes[8], sizes[8] + sizes[9])
    for name, t in (("dw1", 0), ("dw2", 2), ("dw3", 4), ("dw_policy", 10), ("dw_hidden", 12), ("dw_out", 14)):                   # weight gradients: M x N
        assert table[name]["M"] * table[name]["N"] == sizes[t], name
    assert table["dw6"]["M"] * table["dw6"]["N"] == sizes[6] + sizes[7]
    for name, t in (("b1", 1), ("b2", 3), ("b3", 5), ("b_policy", 11), ("b_hidden", 13), ("b_out", 15)):
        c = table["colsum-" + name]
        assert (c["M"], c["N"], c["sam"], c["sak"]) == (1, sizes[t], 0, 0) and c["split"] and c["kslab"] == ks
    assert table["colsum-b6"]["N"] == sizes[8] + sizes[9]
    for name in ("dw1", "dw2", "dw3", "dw6", "colsum-b1", "colsum-b2", "colsum-b3", "colsum-b6"):
        assert table[name]["K"] == rows and table[name]["nz"] == 2 and table[name]["kslab"] == ks          # two k slabs
    for name in ("colsum-b_out", "colsum-b_hidden", "colsum-b_policy"):
        assert table[name]["K"] == n and table[name]["nz"] == 1
    assert (table["dh6-policy"]["cq"], table["dh6-value"]["cq"], table["dh6-value"]["c_off"]) == (sizes[8], sizes[9], sizes[8])
    assert table["dh6-policy"]["cs"] == table["dh6-value"]["cs"] == sizes[8] + sizes[9] and table["dh6-policy"]["ldc"] == 6 * const["kPix"]
    assert "dcol1" not in table and table["dcol3"]["N"] == 9 * 64 and table["dcol2"]["N"] == 9 * 32
    assert {K.variant(c["N"]) for c in table.values()} == {0, 1, 2}


def test_descriptor_wrapper_takes_tensors_or_pointers():
    """gomokuai_amd.lib.train_gemm_desc: a tensor gives its address and what is left of its storage; the defaults are the trainer's gemm()"""
    from gomokuai_amd import lib as G
    t = torch.zeros(40)
    d = G.train_gemm_desc(A=t[8:], B=t.data_ptr() + 4, b_floats=7, M=2, N=3, K=5, sam=5, sak=1)
    assert (d.A, d.a_floats, d.B, d.b_floats) == (t.data_ptr() + 32, 32, t.data_ptr() + 4, 7)
    assert (d.M, d.N, d.K, d.kslab, d.nz, d.z0, d.cq, d.nsplit, d.relu) == (2, 3, 5, 5, 1, 0, K.NONE, K.NONE, 0)
    assert d.part is None and d.C2 is None and d.bias is None and d.mask is None and G.TRAIN_GEMM_NONE == K.NONE
