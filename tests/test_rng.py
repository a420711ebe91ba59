"""Counter-based candidate noise (include/mjpcx.h noise spec). Philox4x32-10 is pinned by the
Random123 known-answer vectors. The Gaussian transform is pinned draw by draw against mpmath, with the nodes every
copy of the candidate noise gives, by tests/sampling_policy_cases.py (tests/test_sampling_policy_cases.py,
tests/test_gpu_sampling_policy.py); the moments below stay as a statistical cross-check of the oracle."""
import ctypes as C

import numpy as np

from mujoco_mpc_amd import capi
from oracle import pyoracle

# Random123 kat_vectors: philox4x32 10 <ctr x4> <key x2> -> <out x4>
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_philox_known_answers():
    for ctr, key, out in KAT:
        assert pyoracle.philox(ctr, key) == out


def test_gaussian_moments():
    z = np.zeros(2)
    zs = []
    for c in range(20000):
        pyoracle.lib().ogaussian_pair(12345, c, 0, 7, z.ctypes.data_as(C.POINTER(C.c_double)))
        zs += [z[0], z[1]]
    zs = np.array(zs)
    assert abs(zs.mean()) < 0.02 and abs(zs.std() - 1) < 0.02
    assert abs(np.mean(zs ** 3)) < 0.06 and abs(np.mean(zs ** 4) - 3) < 0.15


def test_noise_candidates_sampling(cartpole):
    pm = cartpole.packed_model()
    P = 10
    nominal = np.linspace(-0.5, 0.5, P).reshape(P, 1)
    ns = capi.make_noise_spec(seed=1, iteration=3, std0=0.5, nominal_candidate=0)
    out = pyoracle.noise_candidates(pm, ns, P, nominal, range(64))
    assert np.array_equal(out[0], nominal)            # candidate 0 is the un-noised nominal (planner.cc:374)
    assert np.all(np.abs(out) <= 1.0)                 # clamped to ctrlrange
    assert np.std(out[1:] - nominal) > 0.2
    out2 = pyoracle.noise_candidates(pm, ns, P, nominal, range(64))
    assert np.array_equal(out, out2)                  # counter-based: reproducible
    ns2 = capi.make_noise_spec(seed=1, iteration=4, std0=0.5, nominal_candidate=0)
    assert not np.array_equal(out[1:], pyoracle.noise_candidates(pm, ns2, P, nominal, range(64))[1:])


def test_noise_mixture_and_cross_entropy(particle):
    pm = particle.packed_model()
    P, nu = 5, 2
    nominal = np.zeros((P, nu))
    ns = capi.make_noise_spec(seed=5, std0=0.01, std1=0.3, nominal_candidate=-1)
    out = pyoracle.noise_candidates(pm, ns, P, nominal, range(2000))
    big = np.abs(out).reshape(2000, -1).max(axis=1) > 0.06
    assert 0.15 < big.mean() < 0.25                   # ~20 % of candidates use std1 (planner.cc:335-338)
    var = np.full(P * nu, 1e-6); var[3] = 0.04
    ns = capi.make_noise_spec(seed=5, mode=capi.NOISE_CROSS_ENTROPY, std0=0.2, std1=0.01, explore_count=100,
                              nominal_candidate=-1, param_variance=var)
    out = pyoracle.noise_candidates(pm, ns, P, nominal, range(1000)).reshape(1000, -1)
    assert abs(out[100:, 3].std() - 0.2) < 0.03       # sqrt(variance) above the floor
    assert abs(out[100:, 0].std() - 0.01) < 0.003     # std_min floor
    assert abs(out[:100, 0].std() - 0.2) < 0.06       # exploring candidates use std_initial
