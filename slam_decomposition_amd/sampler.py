"""Target distributions (reference: src/slam/sampler.py:20-107)."""
from __future__ import annotations

import logging
import os
import random
import threading
from abc import ABC
from sys import maxsize

import numpy as np
from scipy.stats import unitary_group

from .gates import gate_matrix


def random_unitary(dims: int, seed=None) -> np.ndarray:
    """qiskit ``random_unitary(dims, seed).data`` recipe: SciPy's Haar ``unitary_group`` driven by
    ``np.random.default_rng(seed)``."""
    return unitary_group.rvs(dims, random_state=np.random.default_rng(seed))


class SampleFunction(ABC):
    def __init__(self, n_qubits=2, n_samples=1):
        self.n_qubits = n_qubits
        self.n_samples = n_samples

    def __iter__(self):
        for _ in range(self.n_samples):
            yield self._get_unitary()

    def _get_unitary(self):
        raise NotImplementedError


class GateSample(SampleFunction):
    """src/slam/sampler.py:33-39."""

    def __init__(self, gate, n_samples=1):
        self.gate = gate
        super().__init__(getattr(gate, "num_qubits", 2), n_samples)

    def _get_unitary(self):
        return gate_matrix(self.gate)


class HaarSample(SampleFunction):
    """src/slam/sampler.py:62-71.  Faithful to the reference: Python's ``random`` is re-seeded
    with ``self.seed`` on *every* draw, so an integer seed yields ``n_samples`` identical
    unitaries and ``seed=None`` yields fresh OS entropy each time.
    Use :class:`HaarBatch` for distinct reproducible targets."""

    def __init__(self, seed=None, n_samples=1, n_qubits=2):
        self.seed = seed
        super().__init__(n_samples=n_samples, n_qubits=n_qubits)

    def _get_unitary(self):
        random.seed(self.seed)
        return random_unitary(dims=2**self.n_qubits, seed=random.randint(0, maxsize))


class HaarBatch(SampleFunction):
    """``n_samples`` distinct Haar targets, T_i = random_unitary(4, seed0 + start + i): the
    synthetic benchmark set of SURVEY.md §8(d) (not in the reference)."""

    def __init__(self, seed0: int = 20260000, n_samples: int = 1, start: int = 0, n_qubits=2):
        self.seed0 = int(seed0)
        self.start = int(start)
        super().__init__(n_samples=n_samples, n_qubits=n_qubits)

    def __iter__(self):
        for i in range(self.n_samples):
            yield random_unitary(2**self.n_qubits, seed=self.seed0 + self.start + i)

    def as_array(self) -> np.ndarray:
        return np.stack(list(self))


class DeviceHaarBatch(SampleFunction):
    """``n_samples`` distinct Haar targets generated on the GPU (``slam_sample_haar``): same recipe as
    :class:`HaarSample` (Ginibre -> QR with positive diagonal) but driven by Philox4x32-10 keyed on
    ``(seed, start + i)``, so no host RNG and no upload.  ``TemplateOptimizer`` recognises this sampler
    and leaves the targets on the device; iterating it (like any sampler) copies them back once."""

    def __init__(self, seed: int = 0, n_samples: int = 1, start: int = 0, device: int = 0, n_qubits=2):
        if n_qubits != 2:
            raise NotImplementedError("device sampler: 2 qubits only")
        self.seed = int(seed)
        self.start = int(start)
        self.device = device
        self._cache = None
        super().__init__(n_samples=n_samples, n_qubits=n_qubits)

    def fill(self, ctx, first: int = 0, count=None) -> None:
        """Make this batch -- or its window [first, first + count), one device's shard -- the resident targets of
        ``ctx`` (generated in place)."""
        count = self.n_samples - first if count is None else count
        ctx.sample_haar(self.seed, count, self.start + first)

    def as_array(self) -> np.ndarray:
        if self._cache is None:
            from . import runtime

            ctx = runtime.get_context(self.device)
            self.fill(ctx)
            self._cache = ctx.get_targets(0, self.n_samples)
        return self._cache

    def __iter__(self):
        return iter(self.as_array())


class DeviceHaarSpanBatch(SampleFunction):
    """``n_samples`` Haar targets that are known in advance to need a given number of gates: **the first ``n_samples`` candidates
    at or after ``start`` of the Philox stream ``seed`` whose template size lies in ``span``** -- the reference's ``Haar2Sample`` /
    ``Haar3Sample`` idea (src/slam/sampler.py:73-107: draw, count the gates of the analytic sqrt(iSWAP) pass, discard on a mismatch)
    for any fixed-gate basis, with the draw, the size lookup (the exact regions of ``coverage.py``) and the selection on the device
    (``slam_haar_select_spans``): only the selected candidates' stream indices come back, and ``fill`` regenerates the targets from
    them in place (``slam_sample_haar_indexed``), so every consumer of a device sampler works unchanged.

    ``basis``: a fixed-gate ``CircuitTemplate`` (its gate sequence gives the regions) or a plain list of gate Weyl coordinates in
    circuit order.  ``span``: an int or an inclusive ``(lo, hi)``; the regions of the first ``k_max = max(span)`` gates are used
    (``k_max=`` asks for more, and ``k_max + 1`` then means "out of reach of ``k_max`` gates"; 0 = local targets).  ``margin > 0``
    keeps only candidates whose size does not change when every region is widened or shrunk by ``margin`` (units of pi).

    The selection is lazy and happens once, on ``device``: candidates are scanned in chunks (``chunk=`` fixes the size, otherwise it
    is a guess from the running acceptance rate) until ``n_samples`` are selected -- the batch does not depend on the chunk size.
    Afterwards ``indices`` (int64[n_samples]), ``candidates_scanned`` (up to and including the last taken candidate),
    ``span_counts`` (int64[k_max + 2], over exactly those candidates: their shares estimate the Haar volumes of the prefix
    regions) and ``acceptance`` are available.  ``max_candidates`` (default ``1000 n_samples + 2**20``) scanned without enough
    selected raises ``ValueError`` -- a region of volume 0 (one gate: k = 1) ends this way."""

    MAX_CHUNK = 1 << 24
    MIN_CHUNK = 1 << 12

    def __init__(self, basis, span, seed: int = 0, n_samples: int = 1, start: int = 0, margin: float = 0.0, device: int = 0,
                 chunk=None, max_candidates=None, k_max=None, tol: float = 2e-8, n_qubits=2):
        from . import _ffi

        if n_qubits != 2 or getattr(basis, "n_qubits", 2) != 2:
            raise NotImplementedError("device sampler: 2 qubits only")
        lo, hi = (int(span), int(span)) if np.ndim(span) == 0 else (int(span[0]), int(span[1]))
        if lo > hi:
            raise ValueError(f"span = ({lo}, {hi}): the lower end exceeds the upper")
        if lo < 0:
            raise ValueError(f"span = ({lo}, {hi}): template sizes are >= 0")
        self.k_max = max(hi, 1) if k_max is None else int(k_max)
        if hi > self.k_max + 1:
            raise ValueError(f"span = ({lo}, {hi}) beyond k_max + 1 = {self.k_max + 1} (out of reach of {self.k_max} gates)")
        if self.k_max > _ffi.MAX_SPAN_EVAL:
            raise NotImplementedError(f"template sizes up to {_ffi.MAX_SPAN_EVAL} are looked up on the device (slam_predict_spans); "
                                      f"got {self.k_max}")
        self.gate_coords_seq = self._gate_coords_of(basis, self.k_max)
        self.span = (lo, hi)
        self.seed = int(seed)
        self.start = int(start)
        self.margin = float(margin)
        self.tol = float(tol)
        self.device = device
        if n_samples < 0 or self.start < 0 or self.margin < 0:
            raise ValueError("n_samples, start and margin must be >= 0")
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        self.chunk = None if chunk is None else int(chunk)
        self.max_candidates = 1000 * int(n_samples) + 2**20 if max_candidates is None else int(max_candidates)
        self._lock = threading.Lock()
        self._indices = None
        self._cache = None
        super().__init__(n_samples=int(n_samples), n_qubits=2)

    @staticmethod
    def _gate_coords_of(basis, k_max: int) -> np.ndarray:
        if hasattr(basis, "gate_sequence"):
            if not hasattr(basis, "gate_matrices") or getattr(basis, "mixed_order", False):
                raise NotImplementedError("DeviceHaarSpanBatch conditions on fixed-gate templates (CircuitTemplate): a parametrised "
                                          f"template ({type(basis).__name__}) has no fixed coverage regions")
            from .weyl import c1c2c3

            coords = [c1c2c3(m) for m in basis.gate_matrices]
            return np.array([coords[i] for i in basis.gate_sequence(k_max)], dtype=np.float64).reshape(-1, 3)
        g = np.asarray(basis, dtype=np.float64).reshape(-1, 3)
        if len(g) < k_max:
            raise ValueError(f"{len(g)} gate coordinates given, the span needs {k_max}")
        return g[:k_max].copy()

    # -- selection ---------------------------------------------------------------------------------------------------------------------
    def _next_chunk(self, need: int, scanned: int, taken: int) -> int:
        if self.chunk is not None:
            return self.chunk
        if taken == 0:  # no rate yet: a first guess, then doubled while nothing is found
            guess = max(8 * need, self.MIN_CHUNK) if scanned == 0 else 2 * scanned
        else:
            guess = int(1.1 * need * scanned / taken) + 256
        return min(max(guess, self.MIN_CHUNK), self.MAX_CHUNK)

    def select(self, ctx=None) -> None:
        """Run the selection now (once; later calls return at once) on ``ctx`` (default: the cached context of ``device``)."""
        with self._lock:
            if self._indices is not None:
                return
            if ctx is None:
                from . import runtime

                ctx = runtime.get_context(self.device)
            lo, hi = self.span
            n = self.n_samples
            found = []
            counts = np.zeros(self.k_max + 2, dtype=np.int64)
            taken = scanned = 0
            pos = self.start
            while taken < n:
                if scanned >= self.max_candidates:
                    raise ValueError(f"{scanned} Haar candidates scanned, {taken} of {n} with a template size in {self.span} found "
                                     f"(acceptance {taken / max(scanned, 1):.3g}): max_candidates = {self.max_candidates} reached")
                size = min(self._next_chunk(n - taken, scanned, taken), self.max_candidates - scanned)
                idx, n_sel, part = ctx.haar_select_spans(self.seed, pos, size, self.gate_coords_seq, self.k_max, lo, hi, n - taken,
                                                         tol=self.tol, margin=self.margin)
                if n_sel >= n - taken:
                    # the batch ends inside this chunk: the counts cover the candidates up to the last one taken, not the chunk
                    size = int(idx[-1]) + 1 - pos
                    _, _, part = ctx.haar_select_spans(self.seed, pos, size, self.gate_coords_seq, self.k_max, lo, hi, 0,
                                                       tol=self.tol, margin=self.margin)
                found.append(np.asarray(idx, dtype=np.int64))
                counts += np.asarray(part, dtype=np.int64)
                taken += len(idx)
                scanned += size
                pos += size
            self._scanned = scanned
            self._span_counts = counts
            self._indices = np.concatenate(found) if found else np.zeros(0, dtype=np.int64)

    @property
    def candidates_scanned(self) -> int:
        self.select()
        return self._scanned

    @property
    def span_counts(self) -> np.ndarray:
        self.select()
        return self._span_counts

    @property
    def acceptance(self) -> float:
        self.select()
        return self.n_samples / self._scanned if self._scanned else 0.0

    @property
    def indices(self) -> np.ndarray:
        self.select()
        return self._indices

    # -- the device sampler interface (DeviceHaarBatch) ----------------------------------------------------------------------------
    def fill(self, ctx, first: int = 0, count=None) -> None:
        """Make this batch -- or its window [first, first + count), one device's shard -- the resident targets of ``ctx``
        (regenerated in place from the selected stream indices)."""
        count = self.n_samples - first if count is None else count
        ctx.sample_haar_indexed(self.seed, self.indices[first : first + count])

    def as_array(self) -> np.ndarray:
        if self._cache is None:
            from . import runtime

            if self.n_samples == 0:
                return np.zeros((0, 4, 4), dtype=np.complex128)
            ctx = runtime.get_context(self.device)
            self.fill(ctx)
            self._cache = ctx.get_targets(0, self.n_samples)
        return self._cache

    def __iter__(self):
        return iter(self.as_array())


def _entropy_seed() -> int:
    return int.from_bytes(os.urandom(8), "little")


class _HaarGroundTruth(DeviceHaarSpanBatch):
    """src/slam/sampler.py:73-107: Haar targets that take exactly ``haar_exact`` sqrt(iSWAP) gates.  Deviation from the reference
    (which ignores its seed here: ``random_unitary(dims=4)`` draws from OS entropy): an integer seed gives ``n_samples`` DISTINCT
    reproducible targets (the first ``n_samples`` of the stream with that size); ``seed=None`` takes a seed from OS entropy."""

    haar_exact = 2

    def __init__(self, seed=None, n_samples=1):
        from .gates import RiSwapGate
        from .weyl import c1c2c3

        logging.warning("This sampler only works for \\sqrt[2]iSwap")
        g = c1c2c3(gate_matrix(RiSwapGate(1 / 2)))
        super().__init__([g] * self.haar_exact, self.haar_exact, seed=_entropy_seed() if seed is None else int(seed), n_samples=n_samples)


class Haar2Sample(_HaarGroundTruth):
    haar_exact = 2


class Haar3Sample(_HaarGroundTruth):
    haar_exact = 3
