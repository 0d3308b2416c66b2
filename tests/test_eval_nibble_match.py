"""K1's counter-move rescans ask of a match's record word w0 (pattern_tables.h, DeviceTables::dev_records): is one of its first n_dep
deposit fields -- four bits each from bit 11: the piece index counted from the match's last symbol, bit 3 set for '_' -- the '_' at
index `back`, that is, equal to 8 | back?  eval_kernel.hip's counter_match answers with the zero-nibble test on the sixteen field bits
XOR-ed with 8 | back in every nibble,

    x = ((w0 >> 11) & 0xFFFF) ^ ((8 | back) * 0x1111);   hit = (x - 0x1111) & ~x & 0x8888 & ((1 << 4 n_dep) - 1);   answer: hit != 0

where it used to compare the four fields one by one.  The test flags the lowest zero nibble exactly and may flag nibbles above it that hold
1 (the borrow); "any" only needs that a wrong flag never stands alone inside the mask.  Here: the two statements agree on every record
word the tables hold (the emission lists behind gmk_tables_copy, built into record words as pattern_tables.cpp builds them, first and
second match of every list, every back in 0..7), and on every (back, n_dep in 0..4, 16-bit field) there is.  Exhaustive, exact, no GPU."""
import numpy as np

from gomokuai_amd import lib as G

FIVE = 8


def loop_match(fields, n_dep, back):
    """counter_match's four compares as they stood: d < n_dep and field d == 8 | back, for any d in 0..3 (fields: the sixteen bits, numpy)"""
    hit = np.zeros(fields.shape, dtype=bool)
    for d in range(4):
        f = (fields >> np.uint32(4 * d)) & np.uint32(15)
        hit |= (d < n_dep) & (f == np.uint32(8 | back))
    return hit


def nibble_match(fields, n_dep, back):
    """the kernel's statement, in 32-bit arithmetic that wraps as the device's does"""
    x = (fields & np.uint32(0xFFFF)) ^ np.uint32((8 | back) * 0x1111)
    borrow = (x.astype(np.uint64) + np.uint64((1 << 32) - 0x1111)).astype(np.uint32)       # x - 0x1111 modulo 2^32
    return (borrow & ~x & np.uint32(0x8888) & np.uint32((1 << (4 * n_dep)) - 1)) != 0


def record_words():
    """w0 of both matches of every emission list, as DeviceTables::dev_records holds them"""
    trans, emit, pinfo = G.tables_copy()
    lists = sorted(set(int(t) >> 10 for t in trans) - {0})
    words = []
    for at in lists:
        count = int(emit[at])
        assert 1 <= count <= 2, "a transition reports one or two matches"
        for e in range(count):
            v = int(emit[at + 1 + e])
            p0 = int(pinfo[2 * (v & 0x7FFF)])
            typ, fav, length = p0 & 15, (p0 >> 4) & 1, (p0 >> 5) & 7
            w0, n_dep = typ | fav << 4 | length << 5, 0
            if typ != FIVE:
                for j in range(length):
                    kind = (p0 >> (8 + 2 * j)) & 3                 # piece j from the last symbol: 1 '_', 2 '^'
                    if kind:
                        assert n_dep < 4
                        w0 |= (j | (8 if kind == 1 else 0)) << (11 + 4 * n_dep)
                        n_dep += 1
            w0 |= n_dep << 8 | (v >> 15) << 27
            words.append(w0)
    return np.array(words, dtype=np.uint32)


def test_every_record_word_of_the_tables():
    w0 = record_words()
    n_deps = (w0 >> np.uint32(8)) & np.uint32(7)
    print("%d record words, deposits per word %s" % (len(w0), np.bincount(n_deps, minlength=5).tolist()))
    assert len(w0) >= G.tables_info().n_patterns and n_deps.max() <= 4 and (n_deps > 0).sum() > 100
    fields = (w0 >> np.uint32(11)) & np.uint32(0xFFFF)
    hits = 0
    for back in range(8):
        for n_dep in range(5):
            sel = n_deps == n_dep
            a, b = loop_match(fields[sel], n_dep, back), nibble_match(fields[sel], n_dep, back)
            assert np.array_equal(a, b), "back %d, n_dep %d: record words %s" % (back, n_dep, [hex(w) for w in w0[sel][a != b][:4]])
            hits += int(a.sum())
    print("%d (word, back) pairs hold the '_' asked for" % hits)
    assert hits > 0


def test_every_field_word_back_and_count():
    fields = np.arange(1 << 16, dtype=np.uint32)
    for back in range(8):
        for n_dep in range(5):
            a, b = loop_match(fields, n_dep, back), nibble_match(fields, n_dep, back)
            assert np.array_equal(a, b), "back %d, n_dep %d: fields %s" % (back, n_dep, [hex(f) for f in fields[a != b][:4]])
            assert a.any() == (n_dep > 0)
