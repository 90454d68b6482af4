"""Drive Hamiltonians whose pulse parameters are fitted to a target gate (reference: src/slam/hamiltonian.py) without qutip.

Every class has ``H(*args)`` (an ``ndarray``), a static ``construct_U(*args)`` = exp(-i t H) computed from ``numpy.linalg.eigh``,
``n_params`` / ``parameter_names`` (the arguments of ``construct_U``: what a ``HamiltonianTemplate`` optimises), ``dim`` (4 or 8) and
``device_terms()``, the description the HIP kernels (csrc/slam_ham.hpp) take:

    H(x) = sum_k c_k(x) M_k + h.c.,   c_k = x[s_k] exp(i x[phi_k])   (phi_k = -1: phase 0),   t = x[t_index]   (t_index = -1: t = 1)

with M_k dense dim x dim matrices and all indices positions among ``construct_U``'s arguments.  Operators and basis order are those of
``gates.circulator_hamiltonian``: the raising operator is [[0, 0], [1, 0]] and mode a is the left Kronecker factor.

Piecewise-constant pulses -- ``TimeSliced(h, n_slices, sliced=...)``, ``ConversionGainSmush(n_slices=N)`` and
``ConversionGainSmush1QPhase(n_slices=N)`` -- are products of S slice exponentials exp(-i (t / S) H_s), slice 0 acting first; their
``device_terms()`` carries ``"n_slices"`` and index arrays [S, K] (csrc/slam_hams.hpp), and ``slice_terms(s)`` is slice s alone.
"""
from __future__ import annotations

from inspect import signature

import numpy as np

from .gates import circulator_hamiltonian

MAX_TERMS = 16   # SLAM_HAM_MAX_TERMS
MAX_PARAMS = 32  # SLAM_HAM_MAX_PARAMS
MAX_SLICES = 8   # SLAM_HAMS_MAX_SLICES

_UP = np.array([[0, 0], [1, 0]], dtype=np.complex128)
_ONE = np.eye(2, dtype=np.complex128)


def _modes(n: int):
    """The raising operator on each of n two-level modes, mode 0 the left Kronecker factor."""
    out = []
    for m in range(n):
        op = np.ones((1, 1), dtype=np.complex128)
        for j in range(n):
            op = np.kron(op, _UP if j == m else _ONE)
        out.append(op)
    return out


def expm_hermitian(h: np.ndarray, t: float) -> np.ndarray:
    """exp(-i t h) of a Hermitian h from its eigen-decomposition."""
    w, v = np.linalg.eigh(h)
    return (v * np.exp(-1j * float(t) * w)) @ v.conj().T


def assemble(terms: dict, x) -> np.ndarray:
    """H(x) of a ``device_terms()`` description, term by term in the order and with the operations of ``gates.circulator_hamiltonian``."""
    x = np.asarray(x, dtype=np.float64)
    d = int(terms["dim"])
    h = np.zeros((d, d), dtype=np.complex128)
    for m, s, p in zip(terms["matrices"], terms["s_index"], terms["phi_index"]):
        term = x[s] * np.exp(1j * (x[p] if p >= 0 else 0.0)) * m
        h += term + term.conj().T
    return h


class Hamiltonian:
    """Base class.  ``_TERMS``: per term (operator product, name of the strength argument, name of the phase argument or None), names
    being arguments of ``construct_U``; ``_T``: the name of the time argument or None (t = 1)."""

    dim = 4
    _TERMS = None
    _T = None

    def __repr__(self):
        return type(self).__name__

    @property
    def parameter_names(self):
        return tuple(signature(type(self).construct_U).parameters)

    @property
    def n_params(self) -> int:
        return len(self.parameter_names)

    def _term_matrices(self):
        raise NotImplementedError

    def device_terms(self) -> dict:
        names = self.parameter_names
        mats = self._term_matrices()
        return {
            "dim": self.dim,
            "n_params": len(names),
            "matrices": np.stack(mats),
            "s_index": np.array([names.index(s) for _, s, _ in self._TERMS], dtype=np.int32),
            "phi_index": np.array([-1 if p is None else names.index(p) for _, _, p in self._TERMS], dtype=np.int32),
            "t_index": -1 if self._T is None else names.index(self._T),
        }

    def _H_of_U_args(self, *args) -> np.ndarray:
        """H at ``construct_U``'s arguments (the time among them is ignored)."""
        return assemble(self.device_terms(), np.asarray([float(a) for a in args]))

    def _construct_U_lambda(self, *args):
        return lambda t: expm_hermitian(self.H(*args), t)


class _TwoMode(Hamiltonian):
    dim = 4

    def _term_matrices(self):
        A, B = _modes(2)
        # (x_a, x_b: the single-qubit drives A + h.c., B + h.c.; z_a, z_b: A^+ A and B^+ B, halved because the description adds h.c.)
        ops = {"conv": A @ B.conj().T, "gain": A @ B, "x_a": A, "x_b": B, "z_a": 0.5 * A.conj().T @ A, "z_b": 0.5 * B.conj().T @ B}
        return [ops[o] for o, _, _ in self._TERMS]


class _ThreeMode(Hamiltonian):
    dim = 8

    def _term_matrices(self):
        A, B, C = _modes(3)
        ops = {"conv_ab": A @ B.conj().T, "conv_ac": A @ C.conj().T, "conv_bc": B @ C.conj().T, "gain_ab": A @ B, "gain_ac": A @ C,
               "gain_bc": B @ C}
        return [ops[o] for o, _, _ in self._TERMS]


class SnailEffectiveHamiltonian(_TwoMode):
    """Used to find iSwap family gates: H = geff (A B^+ + h.c.), t = 1 (hamiltonian.py:44-61)."""

    _TERMS = (("conv", "geff", None),)

    def H(self, geff):
        return self._H_of_U_args(geff)

    @staticmethod
    def construct_U(geff):
        return SnailEffectiveHamiltonian()._construct_U_lambda(geff)(1)


class ConversionGainHamiltonian(_TwoMode):
    """Used to find the B gate: H = gc (A B^+ + h.c.) + gg (A B + h.c.), t = 1 (hamiltonian.py:64-81)."""

    _TERMS = (("conv", "gc", None), ("gain", "gg", None))

    def H(self, gc, gg):
        return self._H_of_U_args(gc, gg)

    @staticmethod
    def construct_U(gc, gg):
        return ConversionGainHamiltonian()._construct_U_lambda(gc, gg)(1)


class ConversionGainPhaseHamiltonian(_TwoMode):
    """H(phi_c, phi_g, gc, gg) = gc (e^{i phi_c} A B^+ + h.c.) + gg (e^{i phi_g} A B + h.c.) (hamiltonian.py:84-111).

    Literal reproduction: the reference's ``construct_U(gc, gg, phi_c, phi_g, t=1)`` hands its arguments to ``H`` in ITS order, so the
    first two arguments of ``construct_U`` act as the phases and the next two as the strengths, whatever they are called.  The five
    arguments, t among them, are the template's parameters."""

    _TERMS = (("conv", "phi_c", "gc"), ("gain", "phi_g", "gg"))  # (strength, phase) by the names construct_U gives the positions
    _T = "t"

    def H(self, phi_c, phi_g, gc, gg):
        return self._H_of_U_args(phi_c, phi_g, gc, gg, 1.0)

    @staticmethod
    def construct_U(gc, gg, phi_c, phi_g, t=1):
        return ConversionGainPhaseHamiltonian()._construct_U_lambda(gc, gg, phi_c, phi_g)(float(t))


class CirculatorHamiltonian(_ThreeMode):
    """Use to find VSwap and CParitySwap: ``gates.circulator_hamiltonian`` with a free time (hamiltonian.py:244-272); seven parameters."""

    _TERMS = (("conv_ab", "g_ab", "phi_ab"), ("conv_ac", "g_ac", "phi_ac"), ("conv_bc", "g_bc", "phi_bc"))
    _T = "t"

    def H(self, phi_ab, phi_ac, phi_bc, g_ab, g_ac, g_bc):
        return circulator_hamiltonian(phi_ab, phi_ac, phi_bc, g_ab, g_ac, g_bc)

    @staticmethod
    def construct_U(phi_ab, phi_ac, phi_bc, g_ab, g_ac, g_bc, t):
        return CirculatorHamiltonian()._construct_U_lambda(phi_ab, phi_ac, phi_bc, g_ab, g_ac, g_bc)(float(t))


class DeltaConversionGainHamiltonian(_ThreeMode):
    """Searching for error parity detection gate: conversion (c_*) and gain (g_*) drives on all three pairs, t = 1
    (hamiltonian.py:275-335); twelve parameters.

    Literal reproduction of hamiltonian.py:287-300: the a-b conversion term reads ``cphi_ac`` and ``cphi_ab`` is unused.  So one
    phase feeds two terms, and the derivative with respect to ``cphi_ab`` is identically zero."""

    _TERMS = (("conv_ab", "c_ab", "cphi_ac"), ("gain_ab", "g_ab", "gphi_ab"), ("conv_ac", "c_ac", "cphi_ac"), ("gain_ac", "g_ac", "gphi_ac"),
              ("conv_bc", "c_bc", "cphi_bc"), ("gain_bc", "g_bc", "gphi_bc"))

    def H(self, gphi_ab, gphi_ac, gphi_bc, g_ab, g_ac, g_bc, cphi_ab, cphi_ac, cphi_bc, c_ab, c_ac, c_bc):
        return self._H_of_U_args(gphi_ab, gphi_ac, gphi_bc, g_ab, g_ac, g_bc, cphi_ab, cphi_ac, cphi_bc, c_ab, c_ac, c_bc)

    @staticmethod
    def construct_U(gphi_ab, gphi_ac, gphi_bc, g_ab, g_ac, g_bc, cphi_ab, cphi_ac, cphi_bc, c_ab, c_ac, c_bc):
        return DeltaConversionGainHamiltonian()._construct_U_lambda(gphi_ab, gphi_ac, gphi_bc, g_ab, g_ac, g_bc, cphi_ab, cphi_ac, cphi_bc,
                                                                    c_ab, c_ac, c_bc)(1)


# ---- piecewise-constant pulses: products of slice exponentials ----------------------------------------------------------------------
class _Slices:
    """How the flat parameters of an S-slice pulse map onto the arguments of one slice: ``names`` are the slice Hamiltonian's arguments
    (strengths and phases, the time not among them), ``sliced`` those that get one flat parameter per slice.  Flat order: the shared
    arguments in their order, then per sliced argument (in their order) its S copies ``name0 .. name{S-1}``, then the time."""

    def __init__(self, names, sliced, n_slices, has_time):
        if not (isinstance(n_slices, (int, np.integer)) and 1 <= int(n_slices) <= MAX_SLICES):
            raise ValueError(f"n_slices must be an integer in 1 .. {MAX_SLICES} (got {n_slices!r})")
        sliced = tuple(sliced)
        for name in sliced:
            if name not in names:
                raise ValueError(f"{name!r} is not a strength or phase argument ({', '.join(names)})")
        self.n_slices = S = int(n_slices)
        shared = [a for a in names if a not in sliced]
        per_slice = [a for a in names if a in sliced]
        self.flat_names = tuple(shared + [f"{a}{s}" for a in per_slice for s in range(S)] + (["t"] if has_time else []))
        if len(self.flat_names) > MAX_PARAMS:
            raise ValueError(f"{len(self.flat_names)} parameters: the device takes at most {MAX_PARAMS}")
        # position among the flat parameters of argument `a` in slice s
        self.position = [{a: (shared.index(a) if a in shared else len(shared) + per_slice.index(a) * S + s) for a in names} for s in range(S)]
        self.names = tuple(names)
        self.t_index = len(self.flat_names) - 1 if has_time else -1

    def slice_args(self, x, s):
        return [float(x[self.position[s][a]]) for a in self.names]

    def time(self, x):
        return float(x[self.t_index]) if self.t_index >= 0 else 1.0

    def terms(self, dim, matrices, term_names):
        """``term_names``: per term (strength argument, phase argument or None)"""
        return {
            "dim": dim,
            "n_params": len(self.flat_names),
            "n_slices": self.n_slices,
            "matrices": np.stack(matrices),
            "s_index": np.array([[pos[sn] for sn, _ in term_names] for pos in self.position], dtype=np.int32),
            "phi_index": np.array([[-1 if pn is None else pos[pn] for _, pn in term_names] for pos in self.position], dtype=np.int32),
            "t_index": self.t_index,
        }


def slice_terms(terms: dict, s: int) -> dict:
    """Slice s of a time-sliced description as a description of one exponential (for ``assemble``); its time is the whole pulse's."""
    out = {k: v for k, v in terms.items() if k != "n_slices"}
    out["s_index"], out["phi_index"] = terms["s_index"][s], terms["phi_index"][s]
    return out


class TimeSliced(Hamiltonian):
    """``TimeSliced(h, n_slices, sliced=("g_ab", ...))``: the pulse U = U_S ... U_1, U_s = exp(-i (t / S) H_s), of any Hamiltonian ``h``
    with a device description; the strength or phase arguments named in ``sliced`` take one value per slice (``g_ab0 .. g_ab{S-1}``), the
    others are shared by the slices, and the time, if ``h`` has one, stays last.  With all slices equal it is ``h``."""

    def __init__(self, h, n_slices, sliced=()):
        base = h.device_terms()  # (NotImplementedError for the host-only Hamiltonians)
        names = h.parameter_names
        ti = base["t_index"]
        args = [a for i, a in enumerate(names) if i != ti]
        self.h = h
        self.dim = int(base["dim"])
        self._map = _Slices(args, sliced, n_slices, ti >= 0)
        self.n_slices = self._map.n_slices
        self._base = base
        self._term_names = [(names[s], None if p < 0 else names[p]) for s, p in zip(base["s_index"], base["phi_index"])]
        self._full = lambda a, t: a + [t] if ti >= 0 else a  # (the time is the last argument of every device Hamiltonian that has one)
        assert ti in (-1, len(names) - 1)

    def __repr__(self):
        return f"TimeSliced({self.h!r}, {self.n_slices})"

    @property
    def parameter_names(self):
        return self._map.flat_names

    def device_terms(self) -> dict:
        return self._map.terms(self.dim, self._base["matrices"], self._term_names)

    def H(self, *x, s=0):
        """H of slice s at the flat parameters (the time among them is ignored)"""
        return assemble(self._base, np.asarray(self._full(self._map.slice_args(x, s), 0.0)))

    def construct_U(self, *x):
        S, t = self.n_slices, self._map.time(x)
        total = np.eye(self.dim, dtype=np.complex128)
        for s in range(S):
            total = expm_hermitian(self.H(*x, s=s), t / S) @ total
        return total

    construct_U_flat = construct_U


class _SlicedDrives:
    """What ``ConversionGainSmush(n_slices=N)`` and ``ConversionGainSmush1QPhase(n_slices=N)`` add to the host-only classes: the flat
    parameters (...scalars in the reference's order..., gx0 .. gx{N-1}, gy0 .. gy{N-1}, t), ``construct_U_flat`` and the device description.
    Without ``n_slices`` nothing changes: ``construct_U`` takes the drive vectors and there is no device description."""

    _HOST_ONLY = ""

    def __init__(self, n_slices=None):
        self.n_slices = None
        if n_slices is not None:
            args = tuple(signature(type(self).H).parameters)[1:]
            self._map = _Slices(args, ("gx", "gy"), n_slices, True)
            self.n_slices = self._map.n_slices

    def __repr__(self):
        return type(self).__name__ + ("" if self.n_slices is None else f"(n_slices={self.n_slices})")

    @property
    def parameter_names(self):
        return super().parameter_names if self.n_slices is None else self._map.flat_names

    def device_terms(self) -> dict:
        if self.n_slices is None:
            raise NotImplementedError(self._HOST_ONLY)
        return self._map.terms(self.dim, self._term_matrices(), [(s, p) for _, s, p in self._TERMS])

    def construct_U_flat(self, *x):
        """``construct_U`` at the flat parameters"""
        if self.n_slices is None:
            raise NotImplementedError(self._HOST_ONLY)
        N = self.n_slices
        if len(x) != 2 * N + len(self._map.names) - 2 + 1:
            raise ValueError(f"expected {len(self._map.flat_names)} parameters, got {len(x)}")
        k = len(x) - 2 * N - 1
        return type(self).construct_U(*x[:k], list(x[k:k + N]), list(x[k + N:k + 2 * N]), x[-1])


# ---- host-only classes (import parity): no device description -----------------------------------------------------------------------
class FSimHamiltonian(Hamiltonian):
    """H = g (s+ s- + s- s+) + g^2 / |eta| sz sz (hamiltonian.py:220-241, arXiv:1910.11333)."""

    def H(self, g, eta):
        sp = np.array([[0, 1], [0, 0]], dtype=np.complex128)
        sz = np.diag([1.0, -1.0]).astype(np.complex128)
        h1 = np.kron(sp, _ONE) @ np.kron(_ONE, sp.T) + np.kron(sp.T, _ONE) @ np.kron(_ONE, sp)
        return g * h1 + (g**2 / np.abs(eta)) * np.kron(sz, sz)

    @staticmethod
    def construct_U(g, eta, t=1):
        return FSimHamiltonian()._construct_U_lambda(g, eta)(t)

    def device_terms(self):
        raise NotImplementedError("FSimHamiltonian: the g^2 / |eta| coefficient is not of the form strength * exp(i phase) the device takes")


def _sliced_U(h_of_slice, gxvector, gyvector, t):
    assert len(gxvector) == len(gyvector)
    n = len(gxvector)
    total = np.eye(4, dtype=np.complex128)
    for it in range(n):
        total = expm_hermitian(h_of_slice(gxvector[it], gyvector[it]), t / n) @ total
    return total


class ConversionGainSmush(_SlicedDrives, _TwoMode):
    """Conversion / gain with single-qubit x drives that change from time slice to time slice (hamiltonian.py:114-144).
    ``ConversionGainSmush(n_slices=N)`` has a device description (see ``_SlicedDrives``)."""

    _TERMS = (("x_a", "gx", None), ("x_b", "gy", None), ("conv", "gc", "phi_c"), ("gain", "gg", "phi_g"))
    _HOST_ONLY = "ConversionGainSmush: a product of time slices, not one exp(-i t H) (see parallel_drive.py)"

    def H(self, phi_c, phi_g, gc, gg, gx, gy):
        A, B = _modes(2)
        Ad, Bd = A.conj().T, B.conj().T
        h_c = np.exp(1j * phi_c) * A @ Bd + np.exp(-1j * phi_c) * Ad @ B
        h_g = np.exp(1j * phi_g) * A @ B + np.exp(-1j * phi_g) * Ad @ Bd
        return gx * (A + Ad) + gy * (B + Bd) + gc * h_c + gg * h_g

    @staticmethod
    def construct_U(phi_c, phi_g, gc, gg, gxvector, gyvector, t=1):
        h = ConversionGainSmush()
        return _sliced_U(lambda gx, gy: h.H(phi_c, phi_g, gc, gg, gx, gy), gxvector, gyvector, t)


class ConversionGainSmush1QPhase(_SlicedDrives, _TwoMode):
    """As ConversionGainSmush with phases on the single-qubit drives and z terms (hamiltonian.py:147-182)."""

    _TERMS = (("x_a", "gx", "phi_a"), ("x_b", "gy", "phi_b"), ("conv", "gc", "phi_c"), ("gain", "gg", "phi_g"), ("z_a", "gz1", None),
              ("z_b", "gz2", None))
    _HOST_ONLY = "ConversionGainSmush1QPhase: a product of time slices, not one exp(-i t H) (see parallel_drive.py)"

    def H(self, phi_a, phi_b, phi_c, phi_g, gc, gg, gz1, gz2, gx, gy):
        A, B = _modes(2)
        Ad, Bd = A.conj().T, B.conj().T
        h_x = np.exp(1j * phi_a) * A + np.exp(-1j * phi_a) * Ad
        h_y = np.exp(1j * phi_b) * B + np.exp(-1j * phi_b) * Bd
        h_c = np.exp(1j * phi_c) * A @ Bd + np.exp(-1j * phi_c) * Ad @ B
        h_g = np.exp(1j * phi_g) * A @ B + np.exp(-1j * phi_g) * Ad @ Bd
        return gx * h_x + gy * h_y + gc * h_c + gg * h_g + gz1 * (Ad @ A) + gz2 * (Bd @ B)

    @staticmethod
    def construct_U(phi_a, phi_b, phi_c, phi_g, gc, gg, gz1, gz2, gxvector, gyvector, t=1):
        h = ConversionGainSmush1QPhase()
        return _sliced_U(lambda gx, gy: h.H(phi_a, phi_b, phi_c, phi_g, gc, gg, gz1, gz2, gx, gy), gxvector, gyvector, t)
