"""CPU: the span-conditioned Haar sampler (sampler.DeviceHaarSpanBatch, Haar2Sample / Haar3Sample; slam_haar_select_spans,
slam_sample_haar_indexed) -- everything that needs no GPU: the two symbols, the argument checks, the chunk planner against a stand-in
context, and the host oracle's numbers for the 6000 candidates the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest

import span_sampler_ref as ref
from slam_decomposition_amd import _ffi, sampler
from slam_decomposition_amd.basis import CircuitTemplate
from slam_decomposition_amd.gates import RiSwapGate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("slam_haar_select_spans", "slam_sample_haar_indexed")


def test_the_two_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slam_hip.h")).read(), flags=re.S)
    lib = _ffi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} not declared in slam_hip.h"
        assert name in _ffi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert len(lib.slam_haar_select_spans.argtypes) == 15 and len(lib.slam_sample_haar_indexed.argtypes) == 4
    assert lib.slam_abi_version() == 7
    assert re.search(r"#define\s+SLAM_ABI_VERSION\s+7\b", hdr)
    assert hasattr(_ffi.Context, "haar_select_spans") and hasattr(_ffi.Context, "sample_haar_indexed")


def test_entry_points_reject_bad_arguments_without_a_device():
    """The checks that come before the context is used are not reachable without one; a NULL context is refused with a message."""
    lib = _ffi.load_library()
    one = np.zeros(1, dtype=np.int64)
    assert lib.slam_sample_haar_indexed(None, 1, _ffi._ptr(one), 1) < 0
    assert b"ctx is NULL" in lib.slam_last_error()
    m = ctypes.c_int64(0)
    d = np.zeros(64)
    assert lib.slam_haar_select_spans(None, 1, 0, 1, 3, _ffi._ptr(d), _ffi._ptr(d), 0.0, 0.0, 2, 3, 1, ctypes.byref(m), _ffi._ptr(one), None) < 0
    assert b"ctx is NULL" in lib.slam_last_error()


def test_argument_validation():
    basis = CircuitTemplate(base_gates=[RiSwapGate(1 / 2)])
    b = sampler.DeviceHaarSpanBatch(basis, 3, seed=1, n_samples=5)
    assert b.span == (3, 3) and b.k_max == 3 and np.allclose(b.gate_coords_seq, [ref.SQISWAP] * 3)
    b = sampler.DeviceHaarSpanBatch(basis, (2, 3), n_samples=5)
    assert b.span == (2, 3) and b.k_max == 3 and b.max_candidates == 5000 + 2**20
    # a plain list of Weyl coordinates is the sequence itself
    b = sampler.DeviceHaarSpanBatch(ref.SEQUENCES["iswap_sqiswap2"], 2)
    assert b.k_max == 2 and np.allclose(b.gate_coords_seq, [ref.ISWAP, ref.SQISWAP])
    # k_max + 1 = out of reach of k_max gates
    assert sampler.DeviceHaarSpanBatch(basis, 4, k_max=3).span == (4, 4)
    with pytest.raises(ValueError, match="lower end"):
        sampler.DeviceHaarSpanBatch(basis, (3, 2))
    with pytest.raises(ValueError):
        sampler.DeviceHaarSpanBatch(basis, (-1, 2))
    with pytest.raises(ValueError, match="k_max"):
        sampler.DeviceHaarSpanBatch(basis, 5, k_max=3)
    with pytest.raises(ValueError, match="coordinates"):
        sampler.DeviceHaarSpanBatch([ref.SQISWAP] * 2, 3)
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2

    with pytest.raises(NotImplementedError, match="fixed-gate"):
        sampler.DeviceHaarSpanBatch(CircuitTemplateV2(), 2)
    with pytest.raises(NotImplementedError, match=str(_ffi.MAX_SPAN_EVAL)):
        sampler.DeviceHaarSpanBatch(basis, _ffi.MAX_SPAN_EVAL + 1)
    with pytest.raises(NotImplementedError, match="2 qubits"):
        sampler.DeviceHaarSpanBatch(basis, 2, n_qubits=3)


def test_haar2_and_haar3_are_span_batches_over_sqrt_iswap(caplog):
    with caplog.at_level("WARNING"):
        h2, h3 = sampler.Haar2Sample(seed=5, n_samples=4), sampler.Haar3Sample(n_samples=2)
    assert sum(r.getMessage() == "This sampler only works for \\sqrt[2]iSwap" for r in caplog.records) == 2
    assert isinstance(h2, sampler.DeviceHaarSpanBatch) and isinstance(h3, sampler.SampleFunction)
    assert h2.span == (2, 2) and h3.span == (3, 3) and h2.seed == 5 and h2.n_samples == 4 and h3.n_samples == 2
    assert np.allclose(h2.gate_coords_seq, [ref.SQISWAP] * 2) and np.allclose(h3.gate_coords_seq, [ref.SQISWAP] * 3)
    assert sampler.Haar3Sample().seed != sampler.Haar3Sample().seed  # seed=None: OS entropy


class StubContext:
    """Stands in for _ffi.Context.haar_select_spans: candidate i has span ``spans[i]`` (a fixed pseudo-random table)."""

    def __init__(self, n=4000, k_max=3):
        rng = np.random.default_rng(11)
        self.spans = rng.choice([0, 1, 2, 3, 4], size=n, p=[0.01, 0.0, 0.7, 0.2, 0.09])
        self.calls = []
        self.filled = None

    def haar_select_spans(self, seed, first_index, n_candidates, gate_coords_seq, k_max, span_lo, span_hi, capacity, tol=2e-8, margin=0.0):
        self.calls.append((first_index, n_candidates, capacity))
        assert n_candidates >= 1 and capacity >= 0
        s = np.minimum(self.spans[first_index : first_index + n_candidates], k_max + 1)  # beyond k_max: out of reach
        assert len(s) == n_candidates, "scanned past the stub's stream"
        hit = first_index + np.nonzero((s >= span_lo) & (s <= span_hi))[0]
        return hit[:capacity].astype(np.int64), len(hit), np.bincount(s, minlength=k_max + 2).astype(np.int64)

    def sample_haar_indexed(self, seed, indices):
        self.filled = (seed, np.array(indices))


@pytest.mark.parametrize("chunk", [1, 7, 100000, None])
@pytest.mark.parametrize("start", [0, 123])
def test_chunk_planner_takes_the_first_n_selected_whatever_the_chunk(chunk, start):
    stub = StubContext()
    n = 50
    want = start + np.nonzero(stub.spans[start:] == 3)[0][:n]
    # (a chunk larger than the stream: the budget cuts it to the stream's length)
    b = sampler.DeviceHaarSpanBatch([ref.SQISWAP] * 3, 3, seed=9, n_samples=n, start=start, chunk=chunk, max_candidates=len(stub.spans) - start)
    b.select(stub)
    assert b.indices.dtype == np.int64 and np.array_equal(b.indices, want)
    assert b.candidates_scanned == want[-1] + 1 - start
    assert np.array_equal(b.span_counts, np.bincount(stub.spans[start : want[-1] + 1], minlength=5))
    assert b.acceptance == n / b.candidates_scanned
    n_calls = len(stub.calls)
    b.select(stub)  # once
    assert len(stub.calls) == n_calls
    if chunk == 7:
        assert all(c[1] <= 7 for c in stub.calls)
    b.fill(stub, 10, 5)
    assert stub.filled[0] == 9 and np.array_equal(stub.filled[1], want[10:15])
    b.fill(stub)
    assert np.array_equal(stub.filled[1], want)


def test_max_candidates_raises_and_names_span_and_acceptance():
    stub = StubContext()
    b = sampler.DeviceHaarSpanBatch([ref.SQISWAP], 1, n_samples=3, chunk=64, max_candidates=1000)  # no candidate has span 1
    with pytest.raises(ValueError, match=r"\(1, 1\).*acceptance 0\b.*max_candidates = 1000"):
        b.select(stub)
    assert sum(c[1] for c in stub.calls) == 1000
    stub = StubContext()
    b = sampler.DeviceHaarSpanBatch([ref.SQISWAP] * 3, 3, n_samples=500, max_candidates=1500)  # ~300 of 1500 have span 3
    with pytest.raises(ValueError, match=r"\(3, 3\).*acceptance 0\.[12]"):
        b.select(stub)


def test_host_oracle_counts_for_the_6000_candidates_of_stream_7():
    """coverage.minimal_prefix over three sqrt(iSWAP) gates on haar_philox_port(7, i), i < 6000: 4774 targets of span 2 and 1226 of
    span 3 at tol = 0 (shares 0.7957 / 0.2043; Haar volume of the two-gate region: 0.7901); 19 change span between tol = +2e-4 and
    -2e-4, 0.32 % -- the reference alone stays within the 1 % the GPU tests allow for ambiguous candidates."""
    k0 = ref.host_spans("sqiswap3", 0.0)
    assert np.bincount(k0, minlength=5).tolist() == [0, 0, 4774, 1226, 0]
    amb = ref.host_spans("sqiswap3", 2e-4) != ref.host_spans("sqiswap3", -2e-4)
    assert int(amb.sum()) == 19
    assert amb.mean() <= 0.01
