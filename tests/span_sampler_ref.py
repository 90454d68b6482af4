"""What the span-sampler tests share (tests/test_span_sampler_host.py, tests/test_gpu_span_sampler.py): the gate sequences, and the
host oracle for the 6000 candidates of stream 7 -- the NumPy port of the device generator (oracle.haar_philox_port), their Weyl
coordinates and ``coverage.minimal_prefix`` -- computed once per process and never modified."""
from functools import lru_cache

import numpy as np

SEED = 7
N_CAND = 6000

SQISWAP = (0.25, 0.25, 0.0)
ISWAP = (0.5, 0.5, 0.0)
CX = (0.5, 0.0, 0.0)
SEQUENCES = {"sqiswap3": [SQISWAP] * 3, "cx3": [CX] * 3, "iswap_sqiswap2": [ISWAP, SQISWAP, SQISWAP]}


@lru_cache(maxsize=None)
def port_unitaries() -> np.ndarray:
    from oracle import slam_oracle as o

    u = np.stack([o.haar_philox_port(SEED, i) for i in range(N_CAND)])
    u.setflags(write=False)
    return u


@lru_cache(maxsize=None)
def port_coords() -> np.ndarray:
    from slam_decomposition_amd.weyl import c1c2c3_batch

    c = np.asarray(c1c2c3_batch(port_unitaries()))
    c.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def host_spans(name: str, tol: float) -> np.ndarray:
    from slam_decomposition_amd import coverage

    k = coverage.minimal_prefix(port_coords(), SEQUENCES[name], 3, tol=tol)
    k.setflags(write=False)
    return k
