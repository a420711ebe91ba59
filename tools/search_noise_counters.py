#!/usr/bin/env python3
"""Search the candidate-noise counters (include/mjpcx.h: Philox4x32-10, key = seed, counter = (candidate, pair, iteration, stream)) for the
draws that tests/sampling_policy_cases.py commits as constants (SEARCHED, BERNOULLI_WINDOW): test tooling, not product code.

    stream 0, pair 0   u1 < 1e-6 (|z| > 5); 1 - u1 < 1e-6 (log near 0); u2 within 1e-6 of 0, 1/4, 1/2, 3/4, 1 (roots and extrema)
    stream 1, pair 0   u1 in [0.2, (double)0.2f): the window in which a float comparison of the Bernoulli uniform takes the other std

A vectorised numpy Philox over the global candidate index at a fixed (seed, iteration); about 5e6 draws a second on one core. The test
suite recomputes every constant in Python integers (tests/test_sampling_policy_cases.py), so nothing here is trusted.

    python tools/search_noise_counters.py [--seed S] [--iteration I] [--window-minutes M]"""
import argparse
import time

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of 32-bit words held in uint64"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def k53(hi, lo):
    return ((hi << S32) | lo) >> np.uint64(11)


def draws(first, count, seed, iteration, stream):
    cand = np.arange(first, first + count, dtype=np.uint64)
    zero = np.zeros(count, np.uint64)
    o = philox(cand, zero, zero + np.uint64(iteration), zero + np.uint64(stream), seed)
    return cand, k53(o[0], o[1]), k53(o[2], o[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0001C0FFEE11)
    ap.add_argument("--iteration", type=int, default=3)
    ap.add_argument("--window-minutes", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    a = ap.parse_args()
    two53 = 1 << 53
    eps = int(1e-6 * two53)
    want = {"u1_small": lambda k1, k2: k1 < eps, "u1_near_one": lambda k1, k2: k1 >= two53 - eps}
    for name, q in (("u2_0", 0), ("u2_quarter", two53 // 4), ("u2_half", two53 // 2), ("u2_three_quarters", 3 * (two53 // 4)), ("u2_1", two53)):
        want[name] = (lambda q: lambda k1, k2: np.abs(k2.astype(np.int64) - q) < eps)(q)
    found, first = {}, 1 << 20          # (above 2^20: the same launches cover a large candidate_offset)
    while len(found) < len(want) and first < (1 << 31):
        cand, k1, k2 = draws(first, a.chunk, a.seed, a.iteration, 0)
        for name, f in want.items():
            if name not in found:
                hit = np.flatnonzero(f(k1, k2))
                if hit.size:
                    found[name] = int(cand[hit[0]])
                    print(f'    "{name}": {found[name]},   # k1 = {int(k1[hit[0]])}, k2 = {int(k2[hit[0]])}', flush=True)
        first += a.chunk
    # the Bernoulli window: (2 k + 1) / 2^54 in [0.2, 0.2f)  <=>  k in [ceil(0.2 2^53 - 1/2), ceil(0.2f 2^53 - 1/2))
    from fractions import Fraction
    import math
    lo = math.ceil(Fraction(0.2) * two53 - Fraction(1, 2))
    hi = math.ceil(Fraction(float(np.float32(0.2))) * two53 - Fraction(1, 2))
    t0, first, n = time.time(), 0, 0
    while first < (1 << 31) and time.time() - t0 < 60 * a.window_minutes:
        cand, k1, _ = draws(first, a.chunk, a.seed, a.iteration, 1)
        hit = np.flatnonzero((k1 >= np.uint64(lo)) & (k1 < np.uint64(hi)))
        n += a.chunk
        if hit.size:
            print(f"BERNOULLI_WINDOW = dict(seed={a.seed:#x}, iteration={a.iteration}, candidate={int(cand[hit[0]])})   # k = {int(k1[hit[0]])}, "
                  f"after {n:.3g} draws, {time.time() - t0:.0f} s", flush=True)
            return
        first += a.chunk
    print(f"no Bernoulli window in {n:.3g} draws, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
