"""K11's kernels one at a time, restated in numpy float64 from what include/gomoku_hip.h and train_kernel.hip's headers say they compute --
train_gemm_kernel with its split-K form and its epilogue, train_reduce_kernel, im2col3x3_kernel and col2im3x3_kernel -- together with the case
tables tests/test_train_kernels_gpu.py runs on the device and tests/test_train_kernels_reference.py pins on the CPU.

A CASE is a dict of plain integers and switches (make_case).  materialize(case) turns it into a DESCRIPTOR: the same dict plus the host
buffers A, B, bias, mask (float32, 1-D, starting at the operand's logical element 0, every float no index reaches set to NaN) and the
prefilled outputs C, C2, part (every float SENTINEL).  gemm_ref(desc) gives the outputs' full contents.

Two kinds of data:
  "int"   operands are integers in [-4, 4], biases integers in [-8, 8]: every partial sum is an integer below 2^24 in magnitude for every K
          used here (16 K + 8 < 2^24), so float32 adds them without rounding in ANY order and the comparison is bit for bit;
  "real"  magnitudes 2^e (1 + f), e uniform in [-20, 20), or exact zeros: held to gemm_bound, a derived bound with no constant to tune."""
import zlib

import numpy as np

U = 2.0 ** -24                                     # float32's unit roundoff
TINY = 2.0 ** -126                                 # one flushed subnormal result
NONE = 2 ** 31 - 1                                 # cq / nsplit: no grouping / no split (INT_MAX, as the trainer's gemm() sets them)
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]          # finite (-6.26e18): survives a float64 round trip bit for bit
PIX = 225


# ---------------------------------------------------------------------------------------------------------------- cases
def make_case(name, M, N, K, a="k", b="k", pad=0, split=False, kslab=None, nz=None, z0=0, bias=False, relu=0, mask=False,
              ldc=None, cq=NONE, cs=0, nsplit=NONE, ldc2=None, c_off=0, ldm=None, sam=None, sak=None, sbk=None, sbn=None):
    """a: "k" A[M][K + pad] (k fastest), "m" A[K][M + pad] (m fastest), "0" one element, both strides 0.
    b: "k" B[N][K + pad] (k fastest), "n" B[K][N + pad], "0n" B[K], column stride 0.  Explicit strides override the layout."""
    c = dict(name=name, M=M, N=N, K=K, pad=pad, a=a, b=b)
    c["sam"], c["sak"] = {"k": (K + pad, 1), "m": (1, M + pad), "0": (0, 0)}[a]
    c["sbk"], c["sbn"] = {"k": (1, K + pad), "n": (N + pad, 1), "0n": (1, 0)}[b]
    for key, value in (("sam", sam), ("sak", sak), ("sbk", sbk), ("sbn", sbn)):
        if value is not None:
            c[key] = value
    c["split"] = bool(split)
    c["kslab"] = K if kslab is None else kslab
    c["nz"] = -(-K // c["kslab"]) if nz is None else nz
    c["z0"] = z0
    c["has_bias"], c["relu"], c["has_mask"] = bool(bias), int(relu), bool(mask)
    c["cq"], c["cs"], c["nsplit"], c["c_off"] = cq, cs, nsplit, c_off
    nc = min(N, nsplit)
    c["row_extent"] = 0 if nc == 0 else (nc if cq >= nc else ((nc - 1) // cq) * cs + (nc - 1) % cq + 1)
    c["ldc"] = c["row_extent"] + pad if ldc is None else ldc
    c["ldc2"] = (N - nc) + pad if ldc2 is None else ldc2
    c["ldm"] = N + pad if ldm is None else ldm
    return c


def variant(N):
    """the tile variant launch_gemm picks: 0 for N <= 32 (128 x 32), 1 for N <= 64 (128 x 64), 2 above (128 x 128)"""
    return 0 if N <= 32 else 1 if N <= 64 else 2


M_LIST = (1, 31, 32, 33, 127, 128, 129, 257)
N_LIST = (1, 6, 31, 32, 33, 63, 64, 65, 127, 128, 129, 225, 257)
K_LIST = (1, 2, 3, 15, 16, 17, 31, 33, 450)
# (M, N, K): the first 27 are every (variant of N) x (M mod 32 in 0, 1, 31) x (K mod 16 in 0, 1, 15); the rest bring in the values still missing
EXACT_TRIPLES = (
    (32, 1, 16), (128, 6, 17), (32, 31, 15), (1, 32, 16), (33, 1, 1), (129, 6, 31), (31, 31, 16), (127, 32, 33), (31, 6, 15),
    (128, 33, 16), (32, 63, 17), (128, 64, 31), (257, 33, 16), (1, 64, 33), (33, 63, 15), (127, 64, 16), (31, 33, 1), (127, 63, 31),
    (32, 65, 16), (128, 127, 17), (32, 128, 15), (129, 129, 16), (257, 225, 33), (1, 257, 31), (31, 128, 16), (127, 65, 1), (31, 127, 15),
    (33, 32, 2), (129, 65, 3), (257, 257, 450), (33, 64, 450), (1, 6, 450), (257, 31, 17), (129, 64, 15), (128, 129, 33), (1, 1, 1),
    (257, 128, 16), (32, 32, 16), (33, 33, 33), (127, 225, 2))
SMALL_SHAPES = ((33, 6, 17), (129, 33, 15), (31, 65, 16))                  # one per variant, M and K off the tile


def shape_cases():
    return [make_case("shape-%dx%dx%d" % t, *t) for t in EXACT_TRIPLES]


def layout_cases():
    out = []
    for M, N, K in SMALL_SHAPES:
        for pad in (0, 3):
            for a in "km":
                for b in "kn":
                    out.append(make_case("layout-%dx%dx%d-a%s-b%s-pad%d" % (M, N, K, a, b, pad), M, N, K, a=a, b=b, pad=pad))
            for b in "kn":                         # column_sums' form: M = 1, A is one element
                out.append(make_case("layout-1x%dx%d-a0-b%s-pad%d" % (N, K, b, pad), 1, N, K, a="0", b=b, pad=pad))
            for a in "km":                         # the w_out gradient's form: every column of B is the same vector
                out.append(make_case("layout-%dx%dx%d-a%s-b0n-pad%d" % (M, N, K, a, pad), M, N, K, a=a, b="0n", pad=pad))
            out.append(make_case("layout-%dx%dx1-k1-pad%d" % (M, N, pad), M, N, 1, pad=pad))      # K = 1: sak == 1 and sbk == 1 at once
    out.append(make_case("layout-64x1x9-wout", 64, 1, 9, a="m", b="0n"))
    return out


SPLIT_KSLABS = ((1, 3), (2, 5), (7, 17), (16, 33), (17, 35), (1800, 3607))          # (kslab, a K it does not divide -- but for kslab = 1)
SPLIT_SHAPES = ((33, 6), (31, 33), (129, 65))


def split_cases():
    out = []
    for kslab, K in SPLIT_KSLABS:
        for z0 in (0, 3):
            for i, (M, N) in enumerate(SPLIT_SHAPES):
                out.append(make_case("split-%dx%dx%d-kslab%d-z%d" % (M, N, K, kslab, z0), M, N, K, a="km"[i % 2], b="nk"[(i + z0) % 2],
                                     split=True, kslab=kslab, z0=z0))
    for M, N in SPLIT_SHAPES:                      # the epilogue's switches set: the partials are raw sums all the same
        out.append(make_case("split-%dx%dx17-kslab7-epilogue-ignored" % (M, N), M, N, 17, a="m", b="n", split=True, kslab=7, z0=1,
                             bias=True, relu=1, mask=True))
    return out


REDUCE_MN = ((1, 1), (15, 17), (16, 16), (1, 257), (6, 128))                        # mn = 1, 255, 256, 257, 6 * 128
REDUCE_NZ = ((1, 9, 9), (2, 7, 13), (33, 2, 65))                                    # (nz, kslab, K)


def reduce_cases():
    return [make_case("reduce-mn%d-nz%d" % (M * N, nz), M, N, K, a="m", b="n", split=True, kslab=kslab)
            for M, N in REDUCE_MN for nz, kslab, K in REDUCE_NZ]


def epilogue_cases():
    out = []
    for M, N, K in SMALL_SHAPES:
        out.append(make_case("epi-%dx%dx%d-bias" % (M, N, K), M, N, K, bias=True))
        out.append(make_case("epi-%dx%dx%d-bias-relu" % (M, N, K), M, N, K, bias=True, relu=1))
        out.append(make_case("epi-%dx%dx%d-mask" % (M, N, K), M, N, K, mask=True, pad=2))
        out.append(make_case("epi-%dx%dx%d-bias-relu-mask" % (M, N, K), M, N, K, bias=True, relu=1, mask=True))
    for M in (33, 129):
        # N = 6: ldc = 4 and ldc2 = 2 as the two heads have them; with nsplit = N all six columns of a row go to C, whose rows are then 6 long
        out.append(make_case("epi-%dx6x17-nsplit0" % M, M, 6, 17, bias=True, relu=1, nsplit=0, ldc=4, ldc2=6))
        out.append(make_case("epi-%dx6x17-nsplit4" % M, M, 6, 17, bias=True, relu=1, nsplit=4, ldc=4, ldc2=2))
        out.append(make_case("epi-%dx6x17-nsplit6" % M, M, 6, 17, bias=True, relu=1, nsplit=6, ldc=6, ldc2=2))
    for M in (9, 33):
        out.append(make_case("epi-%dx900x15-cq4-cs6" % M, M, 900, 15, b="n", cq=4, cs=6, ldc=6 * PIX, mask=True, ldm=900))
        out.append(make_case("epi-%dx450x15-cq2-cs6-at4" % M, M, 450, 15, b="n", cq=2, cs=6, ldc=6 * PIX, c_off=4, mask=True, ldm=450))
        out.append(make_case("epi-%dx10x15-cq3-cs5" % M, M, 10, 15, cq=3, cs=5, pad=2))
    out.append(make_case("epi-129x130x17-everything", 129, 130, 17, a="m", b="n", bias=True, relu=1, mask=True, ldm=131,
                         cq=4, cs=6, nsplit=100, ldc=6 * 25 + 1, ldc2=33))
    return out


def trainer_cases(n=9):
    """Every GemmArgs run_forward, run_backward and column_sums build for a batch of n <= 32 positions (one position slab), in call order."""
    rows, ks = n * PIX, 8 * PIX
    out = []

    def colsum(what, K, N):
        out.append(make_case("trainer-colsum-" + what, 1, N, K, a="0", b="n", split=True, kslab=ks))

    for l, (cin, cout) in enumerate(((6, 32), (32, 64), (64, 128)), 1):
        out.append(make_case("trainer-conv%d" % l, rows, cout, 9 * cin, bias=True, relu=1))
    out.append(make_case("trainer-heads", rows, 6, 128, bias=True, relu=1, nsplit=4, ldc=4, ldc2=2))
    out.append(make_case("trainer-logits", n, PIX, 900, bias=True))
    out.append(make_case("trainer-hidden", n, 64, 450, bias=True, relu=1))
    out.append(make_case("trainer-dw_out", 64, 1, n, a="m", b="0n"))
    colsum("b_out", n, 1)
    out.append(make_case("trainer-dw_hidden", 64, 450, n, a="m", b="n"))
    colsum("b_hidden", n, 64)
    out.append(make_case("trainer-dw_policy", PIX, 900, n, a="m", b="n"))
    colsum("b_policy", n, PIX)
    out.append(make_case("trainer-dh6-policy", n, 900, PIX, b="n", cq=4, cs=6, ldc=6 * PIX, mask=True, ldm=900))
    out.append(make_case("trainer-dh6-value", n, 450, 64, b="n", cq=2, cs=6, ldc=6 * PIX, c_off=4, mask=True, ldm=450))
    out.append(make_case("trainer-dw6", 6, 128, rows, a="m", b="n", split=True, kslab=ks))
    colsum("b6", rows, 6)
    out.append(make_case("trainer-dact3", rows, 128, 6, b="n", mask=True, ldm=128))
    for l, (cin, cout) in ((3, (64, 128)), (2, (32, 64)), (1, (6, 32))):
        out.append(make_case("trainer-dw%d" % l, cout, 9 * cin, rows, a="m", b="n", split=True, kslab=ks))
        if l > 1:
            out.append(make_case("trainer-dcol%d" % l, rows, 9 * cin, cout, b="n"))
        colsum("b%d" % l, rows, cout)
    return out


def rounded_cases():
    """Real-valued data.  K = 17 is where the bound is tightest (18 u) and an operand path of lower precision is off by 2^12."""
    return [
        make_case("real-33x31x17", 33, 31, 17),
        make_case("real-129x65x17-am-bn", 129, 65, 17, a="m", b="n", pad=3),
        make_case("real-128x64x16", 128, 64, 16, b="n"),
        make_case("real-257x225x33", 257, 225, 33, a="m"),
        make_case("real-127x63x450-bias", 127, 63, 450, bias=True),
        make_case("real-33x65x3607-split3", 33, 65, 3607, a="m", b="n", split=True, kslab=1800),
        make_case("real-129x33x31-bias-relu-mask", 129, 33, 31, bias=True, relu=1, mask=True),
        make_case("real-31x128x15-bias-relu", 31, 128, 15, bias=True, relu=1, pad=1),
        make_case("real-32x129x450-split-kslab17", 32, 129, 450, split=True, kslab=17, z0=3),
        make_case("real-225x6x128-heads", 225, 6, 128, bias=True, relu=1, nsplit=4, ldc=4, ldc2=2),
        make_case("real-257x33x2", 257, 33, 2, b="n"),
    ]


def exact_cases():
    return shape_cases() + layout_cases() + split_cases() + epilogue_cases()


# ---------------------------------------------------------------------------------------------------------------- data
def _index(s0, n0, s1, n1):
    return np.arange(n0, dtype=np.int64)[:, None] * s0 + np.arange(n1, dtype=np.int64)[None, :] * s1


def index_a(c):
    return _index(c["sam"], c["M"], c["sak"], c["K"])          # [M][K]


def index_b(c):
    return _index(c["sbk"], c["K"], c["sbn"], c["N"])          # [K][N]


def index_mask(c):
    return _index(c["ldm"], c["M"], 1, c["N"])


def index_out(c):
    """direct form -> (to_c2 [M][N] bool, index [M][N] into C or C2); split-K form -> index [nz][M][N] into part"""
    M, N = c["M"], c["N"]
    if c["split"]:
        return (c["z0"] + np.arange(c["nz"], dtype=np.int64))[:, None, None] * (M * N) + _index(N, M, 1, N)[None]
    m, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    to_c2 = np.broadcast_to(n >= c["nsplit"], (M, N))
    in_c = m * c["ldc"] + (n // c["cq"]) * c["cs"] + n % c["cq"]
    in_c2 = m * c["ldc2"] + (n - c["nsplit"])
    return to_c2, np.where(to_c2, in_c2, in_c)


def extents(c):
    """the floats each buffer must hold: its largest index + 1 (0: the descriptor does not use the buffer)"""
    M, N, K = c["M"], c["N"], c["K"]
    e = {"A": (M - 1) * c["sam"] + (K - 1) * c["sak"] + 1, "B": (K - 1) * c["sbk"] + (N - 1) * c["sbn"] + 1,
         "bias": N if c["has_bias"] else 0, "mask": (M - 1) * c["ldm"] + N if c["has_mask"] else 0, "C": 0, "C2": 0, "part": 0}
    if c["split"]:
        e["part"] = (c["z0"] + c["nz"]) * M * N
    else:
        nc = min(N, c["nsplit"])
        e["C"] = (M - 1) * c["ldc"] + c["row_extent"] if nc else 0
        e["C2"] = (M - 1) * c["ldc2"] + (N - nc) if nc < N else 0
    return e


def _values(rng, count, kind, span):
    if kind == "int":
        return rng.integers(-span, span + 1, count).astype(np.float32)
    mag = np.exp2(rng.integers(-20, 20, count).astype(np.float64)) * (1.0 + rng.random(count))
    v = (np.where(rng.random(count) < 0.5, -1.0, 1.0) * mag).astype(np.float32)
    v[rng.random(count) < 0.05] = 0.0
    assert (np.abs(v[v != 0]) >= 2.0 ** -20).all() and (np.abs(v) <= 2.0 ** 20).all()
    return v


MASK_VALUES = np.array([2.0, 0.5, 1e-30, 3.0, 0.0, -0.0, -1.0, np.nan], np.float32)          # only `> 0` keeps: the first four


def _operand(rng, extent, index, kind, span=4):
    buf = np.full(extent, np.nan, np.float32)
    used = np.unique(index)
    buf[used] = _values(rng, used.size, kind, span)
    return buf


def materialize(case, kind="int", seed=0):
    """-> the descriptor: the case plus A, B, bias, mask, C, C2, part and a_floats .. part_floats.  Integer data has no zero in A's last k
    column and B's last k row, so that a dropped last term shows in every element (zeros are everywhere else)."""
    d = dict(case)
    d["kind"] = kind
    rng = np.random.default_rng([zlib.crc32(case["name"].encode()), seed])
    e = extents(case)
    ia, ib = index_a(case), index_b(case)
    d["A"], d["B"] = _operand(rng, e["A"], ia, kind), _operand(rng, e["B"], ib, kind)
    if kind == "int":
        for buf, last in ((d["A"], ia[:, -1]), (d["B"], ib[-1, :])):
            buf[last[buf[last] == 0]] = 1.0
        assert 16 * case["K"] + 8 < 2 ** 24
    d["bias"] = _values(rng, case["N"], kind, 8) if case["has_bias"] else None
    d["mask"] = None
    if case["has_mask"]:
        d["mask"] = np.full(e["mask"], np.nan, np.float32)
        im = index_mask(case)
        d["mask"][im] = MASK_VALUES[rng.integers(0, MASK_VALUES.size, im.shape)]
    for name in ("C", "C2", "part"):
        d[name] = np.full(e[name], SENTINEL, np.float32) if e[name] else None
    for name, key in (("A", "a_floats"), ("B", "b_floats"), ("bias", "bias_floats"), ("mask", "mask_floats"), ("C", "c_floats"),
                      ("C2", "c2_floats"), ("part", "part_floats")):
        d[key] = e[name]
    return d


# ---------------------------------------------------------------------------------------------------------------- the GEMM
def operands(d, dtype=np.float64):
    """-> A [M][K], B [K][N] as the strides define them"""
    return d["A"][index_a(d)].astype(dtype), d["B"][index_b(d)].astype(dtype)


def slabs(d):
    """the k ranges [(k0, k1)] of the nz slabs (the direct form has one that holds every k)"""
    return [(z * d["kslab"], min(d["K"], (z + 1) * d["kslab"])) for z in range(d["nz"])]


def epilogue(d, s, dtype=np.float64):
    """bias, then ReLU, then the mask (keep only where mask > 0), on sums s [M][N] in `dtype`"""
    v = s.astype(dtype)
    if d["bias"] is not None:
        v = v + d["bias"].astype(dtype)[None, :]
    if d["relu"]:
        v = np.maximum(v, dtype(0))
    if d["mask"] is not None:
        with np.errstate(invalid="ignore"):
            v = np.where(d["mask"][index_mask(d)] > 0, v, dtype(0))
    return v


def gemm_logical(d, matmul=None, dtype=np.float64):
    """-> the values the kernel stores: [M][N] after the epilogue (direct form), or [nz][M][N] raw sums (split-K form).  The accumulators
    start at +0.0, so a sum that is zero is +0.0.  `matmul(a, b)`: another product than numpy's in `dtype` (the yardstick tests)."""
    a, b = operands(d, dtype)
    mm = matmul or (lambda x, y: x @ y)
    if d["split"]:
        return np.stack([np.asarray(mm(a[:, k0:k1], b[k0:k1]), dtype) + dtype(0) for k0, k1 in slabs(d)])
    return epilogue(d, np.asarray(mm(a, b), dtype) + dtype(0), dtype) + dtype(0)


def scatter(d, values):
    """the logical values into copies of the prefilled buffers -> {"C", "C2", "part"}: float64 arrays or None, and which floats were written"""
    out = {k: (None if d[k] is None else d[k].astype(np.float64)) for k in ("C", "C2", "part")}
    written = {k: (None if d[k] is None else np.zeros(d[k].size, bool)) for k in ("C", "C2", "part")}
    if d["split"]:
        idx = index_out(d)
        out["part"][idx] = values
        written["part"][idx] = True
    else:
        to_c2, idx = index_out(d)
        for name, sel in (("C", ~to_c2), ("C2", to_c2)):
            if sel.any():
                assert np.unique(idx[sel]).size == sel.sum(), "the store map writes a float twice"
                out[name][idx[sel]] = values[sel]
                written[name][idx[sel]] = True
    return out, written


def gemm_ref(d):
    """-> {"C", "C2", "part"}: the full float64 contents of the output buffers after the call (None for a buffer the form does not use)"""
    return scatter(d, gemm_logical(d))[0]


def gamma(j):
    return j * U / (1.0 - j * U)


def gemm_bound(d):
    """|stored - exact| <= gamma_(K+1) (sum_k |a_mk| |b_kn| + |bias_n|) + 2^-126, in the shape of gemm_logical(d).  K products summed in float32
    in any order, through any number of partials, plus at most one bias add (Higham, Accuracy and Stability of Numerical Algorithms, 3.1);
    ReLU and the mask do not increase a difference.  A split-K slab is held to the sum over its own k."""
    a, b = operands(d)
    a, b = np.abs(a), np.abs(b)
    g = gamma(d["K"] + 1)
    if d["split"]:
        return np.stack([g * (a[:, k0:k1] @ b[k0:k1]) + TINY for k0, k1 in slabs(d)])
    s = a @ b
    if d["bias"] is not None:
        s = s + np.abs(d["bias"].astype(np.float64))[None, :]
    return g * s + TINY


def worst_ratio(d, got_logical):
    """max over the elements of |got - exact| / bound; NaN in `got` counts as infinity"""
    err = np.abs(np.asarray(got_logical, np.float64) - gemm_logical(d))
    ratio = err / gemm_bound(d)
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def gather_logical(d, buffers):
    """from full output buffers {"C", "C2", "part"} (any float type) back to the shape of gemm_logical(d)"""
    if d["split"]:
        return np.asarray(buffers["part"])[index_out(d)]
    to_c2, idx = index_out(d)
    out = np.empty(idx.shape, np.float64)
    for name, sel in (("C", ~to_c2), ("C2", to_c2)):
        if sel.any():
            out[sel] = np.asarray(buffers[name])[idx[sel]]
    return out


def reduce_ref(part, nz, mn):
    """out[i] = part[0][i] + part[1][i] + ... in float32, slab order, from 0.0f"""
    part = np.asarray(part, np.float32).reshape(-1)
    s = np.zeros(mn, np.float32)
    for z in range(nz):
        s = s + part[z * mn:(z + 1) * mn]
    return s


# ---------------------------------------------------------------------------------------------------------------- im2col, col2im
def _taps():
    """for tap t: (pixels p whose tap t lies on the board, the pixel it reads)"""
    y, x = np.divmod(np.arange(PIX), 15)
    out = []
    for t in range(9):
        yy, xx = y + t // 3 - 1, x + t % 3 - 1
        ok = (yy >= 0) & (yy < 15) & (xx >= 0) & (xx < 15)
        out.append((np.nonzero(ok)[0], (yy * 15 + xx)[ok]))
    return out


def im2col_ref(buf, sb, sp, sc, C, npos, dtype=None):
    """col [npos * 225][9 C]: col[b * 225 + p][c * 9 + tap] = the input at (b, the pixel tap / 3 - 1 rows and tap % 3 - 1 columns from p, c),
    0 outside the board; the input element (b, p, c) is buf[b * sb + p * sp + c * sc]"""
    buf = np.asarray(buf)
    col = np.zeros((npos, PIX, C, 9), dtype or buf.dtype)
    src = np.arange(npos)[:, None, None] * sb + np.arange(PIX)[None, :, None] * sp + np.arange(C)[None, None, :] * sc
    for t, (p, q) in enumerate(_taps()):
        col[..., t][:, p, :] = buf[src[:, q, :]]              # (a view of tap t, then the pixels: one advanced index, axes in place)
    return col.reshape(npos * PIX, 9 * C)


def col2im_ref(dcol, C, npos, mask, dtype=np.float32):
    """out [npos * 225][C]: the sum in `dtype`, from 0 and in tap order, of the dcol[row'][c * 9 + tap] whose tap reads the pixel; then 0
    unless mask > 0.  -> (out, sum of the terms' magnitudes in float64)"""
    d = np.asarray(dcol).reshape(npos, PIX, C, 9)
    s, mag = np.zeros((npos, PIX, C), dtype), np.zeros((npos, PIX, C))
    for t, (p, q) in enumerate(_taps()):          # output pixel p reads q through tap t: its gradient goes back to q
        term = d[..., t][:, p, :]
        s[:, q, :] = s[:, q, :] + term.astype(dtype)
        mag[:, q, :] += np.abs(term.astype(np.float64))
    with np.errstate(invalid="ignore"):
        keep = np.asarray(mask).reshape(npos, PIX, C) > 0
    return np.where(keep, s, dtype(0)).reshape(npos * PIX, C), np.where(keep, mag, 0.0).reshape(npos * PIX, C)


CONV_C = (1, 5, 6, 32)
CONV_NPOS = (1, 2, 3)
