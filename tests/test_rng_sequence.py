"""The LCG's cycle of triples (the RNG pre-pass's cycle table, rfx.h rfx_renderer_set_rng_prepass).

randomInsideSphere (reference src/common/Vector3.cpp:176-188) consumes fastrand (trace_math.h:34-39) three draws at
a time, and whether a triple is accepted depends on the state before it alone.  Three draws are one affine map mod
2^32; these tests check on the host that the map has full period, and that the library's discrete logarithm
(rfx_rng_triple_index: the index k of a state in the cycle that starts at state 0) inverts jumping k triples.
"""
import numpy as np

from reflaxman_amd import _lib

A1, C1 = 214013, 2531011  # trace_math.h:36
M = 1 << 32
ORIGIN = 0


def affine_pow(a, c, n):
    """(A, C) of x -> a x + c applied n times, mod 2^32."""
    A, C = 1, 0
    while n:
        if n & 1:
            A, C = (a * A) % M, (a * C + c) % M
        c, a, n = (a * c + c) % M, (a * a) % M, n >> 1
    return A, C


A3, C3 = affine_pow(A1, C1, 3)  # one triple


def jump_triples(s, k):
    A, C = affine_pow(A3, C3, k)
    return (A * s + C) % M


def test_triple_map_has_full_period():
    """Hull-Dobell for modulus 2^32: the increment is odd (coprime to the modulus) and multiplier - 1 is divisible by 4
    (by every prime factor of the modulus, and by 4 as the modulus is)."""
    assert (A3, C3) == ((A1 ** 3) % M, (C1 * (A1 * A1 + A1 + 1)) % M)
    assert C3 % 2 == 1
    assert (A3 - 1) % 4 == 0
    # and so for the single draw, whose cube it is
    assert C1 % 2 == 1 and (A1 - 1) % 4 == 0


def test_index_round_trip():
    L = _lib.load()
    rng = np.random.default_rng(20261019)
    states = [0, 1, M - 1, ORIGIN] + [int(v) for v in rng.integers(0, M, 4000, dtype=np.uint64)]
    for s in states:
        k = L.rfx_rng_triple_index(s)
        assert 0 <= k < M
        assert jump_triples(ORIGIN, k) == s, (s, k)
    assert L.rfx_rng_triple_index(ORIGIN) == 0


def test_index_equals_stepping_from_the_origin():
    L = _lib.load()
    s = ORIGIN
    for k in range(10000):
        assert L.rfx_rng_triple_index(s) == k, k
        for _ in range(3):
            s = (A1 * s + C1) % M
    # the far end of the cycle: the state one triple before the origin
    assert jump_triples(jump_triples(ORIGIN, M - 1), 1) == ORIGIN
    assert L.rfx_rng_triple_index(jump_triples(ORIGIN, M - 1)) == M - 1
