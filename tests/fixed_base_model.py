"""Pure-Python model of the fixed-base multiplication's digit recoding and table indexing
(csrc/mbls_fixed_base.hpp), and the edge scalars its tests share.

k < r in signed radix 2^c: window w is the c bits of k from bit c w on plus the carry from below; a
value >= 2^(c-1) becomes value - 2^c with a carry of one, except in the top window, which keeps its
carry.  table[w 2^(c-1) + d - 1] = [d 2^(c w)] base for d = 1 .. 2^(c-1)."""
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def windows(c):
    return -(-255 // c)


def recode(k, c):
    """the W signed digits of k mod r, lowest window first"""
    k %= R
    W, half, full = windows(c), 1 << (c - 1), 1 << c
    digits, carry = [], 0
    for w in range(W):
        raw = ((k >> (c * w)) & (full - 1)) + carry
        if w < W - 1 and raw >= half:
            digits.append(raw - full)
            carry = 1
        else:
            digits.append(raw)
            carry = 0
    return digits


def table_index(w, d, c):
    """the table row of digit d != 0 in window w"""
    return w * (1 << (c - 1)) + abs(d) - 1


def table_scalar(index, c):
    """the multiple of the base that table row `index` holds"""
    rows = 1 << (c - 1)
    return (index % rows + 1) << (c * (index // rows))


def partial_sums(digits, c):
    """(partial sum before window w, addend of window w) for every non-zero digit, in the order the
    kernel adds them (lowest window first)"""
    acc, out = 0, []
    for w, d in enumerate(digits):
        if d == 0:
            continue
        addend = d << (c * w)
        out.append((acc, addend))
        acc += addend
    return out


def meets_exception(digits, c):
    """does the accumulation add a point to itself or to its negative (a base of order r)?  The
    first addend initialises the accumulator, so its partial sum 0 is not an addition."""
    for acc, addend in partial_sums(digits, c)[1:]:
        if (acc - addend) % R == 0 or (acc + addend) % R == 0:
            return True
    return False


def edge_scalars(c, n_random=64, seed=0xF1BA5E):
    """the edge scalars of the GPU tests: below 300 for c = 8"""
    W, half, full = windows(c), 1 << (c - 1), 1 << c
    sc = [0, 1, 2, R - 1, R, R + 1, (1 << 256) - 1]
    for w in range(W):
        sc += [1 << (c * w), (1 << (c * w)) - 1, half << (c * w), (half - 1) << (c * w)]
    # every window 0x80.., 0x7f.. and 0xff..: the carry through every window
    # (over all W windows the value passes r and is reduced; over the W - 1 below the top it is not)
    sc += [sum(v << (c * w) for w in range(W)) for v in (half, half - 1, full - 1)]
    sc += [sum(v << (c * w) for w in range(W - 1)) for v in (half, half - 1, full - 1)]
    # the largest top digit: the top window's bits of r - 1 with a carry from below
    top = (R - 1) >> (c * (W - 1))
    below = (1 << (c * (W - 1))) - 1
    sc += [(top << (c * (W - 1))) | (half << (c * (W - 2))), (top << (c * (W - 1))) | (below & (R - 1)), R - 2, R - half,
           R - full]
    sc = [s & ((1 << 256) - 1) for s in sc]  # 32-byte scalars (wider only for a c that does not divide 256)
    rnd = random.Random(seed)
    sc += [rnd.randrange(R) for _ in range(n_random)]
    return sc
