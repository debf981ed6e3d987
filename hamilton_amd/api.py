"""Host-side mirror of `Numeric.Hamilton` over the C ABI of libhamk.so.

Same names, argument order and meaning as the reference's export list
(/root/reference/src/Numeric/Hamilton.hs:28-70); the one semantic extension is
that every state may be an ENSEMBLE: positions/velocities/momenta are arrays of
shape [n] (one trajectory, the reference's case) or [n, B] (B independent
trajectories, structure-of-arrays).  numpy arrays take the host-staged path
(HAMK_MEM_HOST); torch CUDA tensors are used in place on the GPU
(HAMK_MEM_DEVICE, launched on torch's current stream).

Python cannot spell a prime: `mkSystem'` is `mkSystem_`, `evolveHam'` is
`evolveHam_`, `evolveHamC'` is `evolveHamC_`.

Error behaviour: API misuse / toolchain / HIP failures raise `HamkError` (the
reference raises Haskell exceptions: Hamilton.hs:425,444,462).  A singular mass
matrix does NOT raise for ensembles: the per-trajectory status word is kept in
`System.last_status` (bit HAMK_ST_SINGULAR) and the affected lanes hold NaN --
for a single trajectory ([n]-shaped input) `SingularSystem` is raised, matching
hmatrix's exception out of `inv` (Hamilton.hs:321,381).
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence
import contextlib

import numpy as np

from . import _abi
from . import tracer as T
from ._abi import HamkError, MEM_DEVICE, MEM_HOST, ST_DRIFT, ST_SINGULAR

try:  # torch is plumbing (device memory, streams); the package works without it on host arrays
    import torch
except Exception:  # pragma: no cover
    torch = None

U_GENERALIZED, U_CARTESIAN = 0, 1


class SingularSystem(ArithmeticError):
    """K = J^T M J not invertible for a single-trajectory call."""


# ---------------------------------------------------------------------------------------
# array plumbing
# ---------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


class _Arr:
    """A [rows, B] fp64 array on host (numpy) or device (torch.cuda)."""

    def __init__(self, data, rows: int, name: str):
        self.single = False
        if _is_torch(data) and data.is_cuda:
            t = data
            if t.dtype != torch.float64:
                t = t.to(torch.float64)
            if t.dim() == 1:
                t = t.reshape(rows, 1)
                self.single = True
            if t.dim() != 2 or t.shape[0] != rows:
                raise ValueError(f"{name}: expected shape [{rows}] or [{rows}, B], got {tuple(data.shape)}")
            self.a = t.contiguous()
            self.device = True
        else:
            a = data.detach().cpu().numpy() if _is_torch(data) else np.asarray(data, dtype=np.float64)
            if a.ndim == 1:
                a = a.reshape(rows, 1)
                self.single = True
            if a.ndim != 2 or a.shape[0] != rows:
                raise ValueError(f"{name}: expected shape [{rows}] or [{rows}, B], got {np.shape(data)}")
            self.a = np.ascontiguousarray(a, dtype=np.float64)
            self.device = False
        self.B = int(self.a.shape[1])

    @property
    def ptr(self):
        return self.a.data_ptr() if self.device else self.a.ctypes.data

    @property
    def mem(self):
        return MEM_DEVICE if self.device else MEM_HOST

    def like(self, rows: Optional[int] = None, dtype="f8", lead: Sequence[int] = (), zero: bool = False):
        """An output array beside this one; zero=True where a call may legally return without writing it."""
        shape = tuple(lead) + ((rows, self.B) if rows is not None else (self.B,))
        if self.device:
            dt = torch.float64 if dtype == "f8" else torch.int32
            return (torch.zeros if zero else torch.empty)(shape, dtype=dt, device=self.a.device)
        return (np.zeros if zero else np.empty)(shape, dtype=np.float64 if dtype == "f8" else np.int32)

    def clone(self):
        return self.a.clone() if self.device else self.a.copy()


def _pair(a, name_a: str, b, name_b: str, rows: int):
    """Two arrays of one state (positions + velocities / momenta): same ensemble size, same place."""
    xa, xb = _Arr(a, rows, name_a), _Arr(b, rows, name_b)
    if xa.B != xb.B or xa.single != xb.single:
        raise ValueError(f"{name_a} and {name_b} describe different ensembles ({xa.B} vs {xb.B} trajectories)")
    if xa.device != xb.device or (xa.device and xa.a.device != xb.a.device):
        raise ValueError(f"{name_a} and {name_b} must live in the same memory (both host arrays or both tensors of one GPU)")
    return xa, xb


def _in_place(x: "_Arr", original, name: str):
    """inplace=True only makes sense if the array handed to the library IS the caller's array."""
    same = (x.a.data_ptr() == original.data_ptr()) if (x.device and _is_torch(original)) else \
        (isinstance(original, np.ndarray) and x.a.ctypes.data == original.ctypes.data)
    if not same:
        raise ValueError(f"inplace=True needs {name} as a contiguous float64 [n, B] array (a converted copy would be advanced instead)")


def _ptr(x):
    if x is None:
        return None
    return x.data_ptr() if _is_torch(x) else x.ctypes.data


def _shape_out(x, single: bool):
    """[rows, 1] -> [rows] (and [1] -> scalar) when the caller passed one trajectory."""
    if not single:
        return x
    if x.ndim == 1:
        return float(x[0])
    return x[..., 0]


# ---------------------------------------------------------------------------------------
# Systems and states                                              Hamilton.hs:103-169
# ---------------------------------------------------------------------------------------
class Config:
    """`Cfg { cfgPositions, cfgVelocities }` (Hamilton.hs:103-115)."""

    def __init__(self, positions, velocities):
        self.positions = positions
        self.velocities = velocities

    cfgPositions = property(lambda self: self.positions)
    cfgVelocities = property(lambda self: self.velocities)

    def __repr__(self):
        return f"Cfg {{cfgPositions = {self.positions!r}, cfgVelocities = {self.velocities!r}}}"


class Phase:
    """`Phs { phsPositions, phsMomenta }` (Hamilton.hs:133-145)."""

    def __init__(self, positions, momenta):
        self.positions = positions
        self.momenta = momenta

    phsPositions = property(lambda self: self.positions)
    phsMomenta = property(lambda self: self.momenta)

    def __repr__(self):
        return f"Phs {{phsPositions = {self.positions!r}, phsMomenta = {self.momenta!r}}}"


Cfg, Phs = Config, Phase


class System:
    """Opaque `System m n` (Hamilton.hs:160-169): owns a libhamk handle."""

    def __init__(self, m: int, n: int, inertia, tape_f: T.Tape, tape_u: T.Tape, u_space: int, options=None):
        """options: a `hamilton_amd._abi.HamkOptions` or a dict of its fields (hamk.h `hamk_options`; unset = the
        library's own choice) -- which lanes serve a trajectory, AD strategy, stepping bodies, sincos policy, GSL
        binding, self-check ...  Environment variables remain as test overrides of whatever is left to the library."""
        self.m, self.n = int(m), int(n)
        self.u_space = u_space
        self.tape_f, self.tape_u = tape_f, tape_u
        self.last_status = None
        self.last_nsub = None
        L = _abi.lib()
        f_ops, f_n, f_outs = tape_f.as_ctypes()
        u_ops, u_n, _ = tape_u.as_ctypes()
        w = (ctypes.c_double * self.m)(*[float(v) for v in inertia])
        h = ctypes.c_void_p()
        if isinstance(options, dict):
            options = _abi.HamkOptions(**options)
        _abi.check(L.hamk_system_create_ex(self.m, self.n, w, f_ops, f_n, f_outs, u_ops, u_n, tape_u.outs[0],
                                           u_space, ctypes.byref(options) if options is not None else None, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _abi.lib().hamk_system_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def options(self, B: int = -1) -> dict:
        """What a launch over B trajectories uses (B < 0: a large ensemble), every choice resolved
        (hamk_system_get_options): mapping, ad_mode, bodies, trig, ..., lanes_per_trajectory."""
        o = _abi.HamkOptions()
        _abi.check(_abi.lib().hamk_system_get_options(self._h, int(B), ctypes.byref(o)))
        return o.as_dict()

    def set_ensemble_size(self, total: int):
        """The size of the WHOLE ensemble this handle's launches are pieces of (hamk_system_set_ensemble_size): the library
        then picks the mapping for that size instead of each launch's own -- shards, chunks and resumed runs reproduce the
        one-launch bits whatever the split.  0: back to per-launch choice."""
        _abi.check(_abi.lib().hamk_system_set_ensemble_size(self._h, int(total)))
        return self

    def describe_batch(self, B: int = -1):
        """`source`, `build_info`, `code_size`, `code_object`, `kernel_bytes` below describe the specialisation a launch
        over B trajectories uses (default: the one built at creation = the large-ensemble one)."""
        _abi.check(_abi.lib().hamk_system_describe_batch(self._h, int(B)))
        return self

    @property
    def lanes_per_trajectory(self) -> int:
        """1 (lane kernels), 4 (quad), 16 / 32 / 64 (wave-cooperative) -- of the specialisation being described."""
        src = self.source
        if "HAMK_INSTANTIATE_WAVE" in src:
            return 16 if self.n <= 16 else (32 if self.n <= 32 else 64)
        return 4 if "HAMK_INSTANTIATE_QUAD" in src else 1

    @property
    def source(self) -> str:
        return _abi.lib().hamk_system_source(self._h).decode()

    @property
    def build_info(self) -> str:
        return _abi.lib().hamk_system_build_info(self._h).decode()

    @property
    def code_size(self) -> int:
        return int(_abi.lib().hamk_system_code_size(self._h))

    def _symplectic_text(self, fn) -> str:
        """A `const char*` return carries no code: NULL means hamk_last_error() says why.  The code of the exception is read off
        that text -- the stepper refused for this handle (n > 16, another mapping stated: HAMK_ERR_UNSUPPORTED), else a failed
        build of the companion module (HAMK_ERR_COMPILE)."""
        text = fn(self._h)
        if text is None:
            msg = _abi.lib().hamk_last_error().decode("utf-8", "replace")
            unsupported = msg.startswith(("the symplectic stepper", "the Lyapunov stepper", "the Poincare-section stepper", "the exit-time stepper", "the recording stepper")) or "unsupported" in msg
            raise HamkError(_abi.HAMK_ERR_UNSUPPORTED if unsupported else _abi.HAMK_ERR_COMPILE, msg)
        return text.decode()

    @property
    def symplectic_source(self) -> str:
        """Source of the symplectic stepper's companion module (hamk_symplectic_source; builds it if needed, needs no GPU)."""
        return self._symplectic_text(_abi.lib().hamk_symplectic_source)

    @property
    def symplectic_build_info(self) -> str:
        """One `build_info`-format line for hamk_symp_steps_k: bytes, spilled SGPRs / VGPRs, allocated VGPRs."""
        return self._symplectic_text(_abi.lib().hamk_symplectic_build_info)

    @property
    def lyapunov_source(self) -> str:
        """Source of the Lyapunov stepper's companion module (hamk_lyapunov_source; builds it if needed, needs no GPU)."""
        return self._symplectic_text(_abi.lib().hamk_lyapunov_source)

    @property
    def lyapunov_build_info(self) -> str:
        """One `build_info`-format line for hamk_lyap_steps_k: bytes, spilled SGPRs / VGPRs, allocated VGPRs, function symbols."""
        return self._symplectic_text(_abi.lib().hamk_lyapunov_build_info)

    @property
    def poincare_source(self) -> str:
        """Source of the Poincare-section stepper's companion module (hamk_poincare_source; builds it if needed, needs no GPU)."""
        return self._symplectic_text(_abi.lib().hamk_poincare_source)

    @property
    def poincare_build_info(self) -> str:
        """One `build_info`-format line for hamk_psec_steps_k: bytes, spilled SGPRs / VGPRs, allocated VGPRs, function symbols."""
        return self._symplectic_text(_abi.lib().hamk_poincare_build_info)

    @property
    def exit_source(self) -> str:
        """Source of the exit-time stepper's companion module (hamk_exit_source; builds it if needed, needs no GPU)."""
        return self._symplectic_text(_abi.lib().hamk_exit_source)

    @property
    def exit_build_info(self) -> str:
        """One `build_info`-format line for hamk_exit_steps_k: bytes, spilled SGPRs / VGPRs, allocated VGPRs, function symbols."""
        return self._symplectic_text(_abi.lib().hamk_exit_build_info)

    @property
    def record_source(self) -> str:
        """Source of the recording stepper's companion module (hamk_record_source; builds it if needed, needs no GPU)."""
        return self._symplectic_text(_abi.lib().hamk_record_source)

    @property
    def record_build_info(self) -> str:
        """One `build_info`-format line for hamk_rec_steps_k: bytes, spilled SGPRs / VGPRs, allocated VGPRs, function symbols."""
        return self._symplectic_text(_abi.lib().hamk_record_build_info)

    def kernel_bytes(self, kernel: str) -> int:
        return int(_abi.lib().hamk_system_kernel_bytes(self._h, kernel.encode()))

    @property
    def num_device_functions(self) -> int:
        return int(_abi.lib().hamk_system_kernel_bytes(self._h, None))

    def synchronize(self):
        _abi.check(_abi.lib().hamk_synchronize(self._h))

    @contextlib.contextmanager
    def _on(self, arr: _Arr):
        """Run the enclosed libhamk call where `arr` lives: a handle launches on the calling thread's
        CURRENT device (hamk.h), so tensors of cuda:1 need cuda:1 current for the duration of the
        call -- on torch's current stream of that device.  The handle keeps one module / staging
        state per device, so alternating devices costs nothing after the first use of each."""
        if arr.device:
            with torch.cuda.device(arr.a.device):
                stream = torch.cuda.current_stream(arr.a.device).cuda_stream
                _abi.check(_abi.lib().hamk_set_stream(self._h, ctypes.c_void_p(stream)))
                yield
        else:
            _abi.check(_abi.lib().hamk_set_stream(self._h, None))
            yield

    @property
    def gsl_api(self) -> int:
        """Which binding of hmatrix-gsl's gsl-ode.c stepHam / evolveHam follow: 2 = gsl_odeiv2
        driver (its default build, this library's default), 1 = old gsl_odeiv (-DGSLODE1).  hamk.h."""
        return int(_abi.lib().hamk_system_get_gsl_api(self._h))

    @gsl_api.setter
    def gsl_api(self, api: int):
        _abi.check(_abi.lib().hamk_system_set_gsl_api(self._h, int(api)))

    def code_object(self, which: int = 0) -> bytes:
        """The gfx950 ELF the kernels are loaded from (which = 1: the build without MachineLICM)."""
        L = _abi.lib()
        n = int(L.hamk_system_code_object(self._h, which, None, 0))
        if n == 0:
            return b""
        buf = ctypes.create_string_buffer(n)
        L.hamk_system_code_object(self._h, which, buf, n)
        return buf.raw

    def _after(self, status, single: bool, what: str):
        self.last_status = status
        if single and status is not None:
            st = int(status[0])
            if st & ST_SINGULAR:
                raise SingularSystem(f"{what}: mass matrix J^T M J is singular")


def mkSystem(inertia, f: Callable, u: Callable, n: int, options=None) -> System:
    """mkSystem (Hamilton.hs:201-225): potential over GENERALIZED coordinates.

    `f(q)` maps a list of n values to m values, `u(q)` to a scalar; both written
    against hamilton_amd's traced arithmetic (the `RealFloat a` of the reference).
    m = len(inertia); n cannot be read off a Python function and is explicit."""
    m = len(inertia)
    return System(m, n, inertia, T.trace(f, n, m), T.trace(u, n, None), U_GENERALIZED, options)


def mkSystem_(inertia, f: Callable, u: Callable, n: int, options=None) -> System:
    """mkSystem' (Hamilton.hs:238-254): potential over the underlying CARTESIAN coordinates."""
    m = len(inertia)
    return System(m, n, inertia, T.trace(f, n, m), T.trace(u, m, None), U_CARTESIAN, options)


def system_from_spec(spec, options=None) -> System:
    """Build a System from a hamilton_amd.examples.SystemSpec."""
    tf, tu = spec.trace()
    return System(spec.m, spec.n, spec.inertia, tf, tu, spec.u_space, options)


# ---------------------------------------------------------------------------------------
# state functions
# ---------------------------------------------------------------------------------------
def underlyingPos(s: System, q):
    """underlyingPos (Hamilton.hs:174-178)."""
    qa = _Arr(q, s.n, "positions")
    x = qa.like(s.m)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_coords_batch(s._h, qa.B, qa.ptr, _ptr(x), qa.mem))
    return _shape_out(x, qa.single)


def momenta(s: System, c: Config):
    """momenta (Hamilton.hs:262-269)."""
    qa, va = _pair(c.positions, "positions", c.velocities, "velocities", s.n)
    p = qa.like(s.n)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_to_phase_batch(s._h, qa.B, qa.ptr, va.ptr, _ptr(p), qa.mem))
    return _shape_out(p, qa.single)


def toPhase(s: System, c: Config) -> Phase:
    """toPhase (Hamilton.hs:279-284)."""
    return Phase(c.positions, momenta(s, c))


def velocities(s: System, ph: Phase):
    """velocities (Hamilton.hs:316-324)."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    v, st = qa.like(s.n), qa.like(None, "i4")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_from_phase_batch(s._h, qa.B, qa.ptr, pa.ptr, _ptr(v), _ptr(st), qa.mem))
    s._after(st, qa.single, "velocities")
    return _shape_out(v, qa.single)


def fromPhase(s: System, ph: Phase) -> Config:
    """fromPhase (Hamilton.hs:332-337)."""
    return Config(ph.positions, velocities(s, ph))


def _observe(s: System, q, p, which: str):
    if p is not None:
        qa, pa = _pair(q, "positions", p, "momenta", s.n)
    else:
        qa, pa = _Arr(q, s.n, "positions"), None
    out, st = qa.like(None), qa.like(None, "i4")
    ptrs = {"ke": None, "pe": None, "h": None}
    ptrs[which] = _ptr(out)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_observe_batch(s._h, qa.B, qa.ptr, pa.ptr if pa is not None else None,
                                                 ptrs["ke"], ptrs["pe"], ptrs["h"], _ptr(st), qa.mem))
    if which != "pe":
        s._after(st, qa.single, which)
    return _shape_out(out, qa.single)


def keP(s: System, ph: Phase):
    """keP (Hamilton.hs:341-349)."""
    return _observe(s, ph.positions, ph.momenta, "ke")


def hamiltonian(s: System, ph: Phase):
    """hamiltonian (Hamilton.hs:353-361)."""
    return _observe(s, ph.positions, ph.momenta, "h")


def pe(s: System, q):
    """pe (Hamilton.hs:182-186)."""
    return _observe(s, q, None, "pe")


def _observe_config(s: System, c: Config, which: str):
    qa, va = _pair(c.positions, "positions", c.velocities, "velocities", s.n)
    out = qa.like(None)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_observe_config_batch(
            s._h, qa.B, qa.ptr, va.ptr, _ptr(out) if which == "ke" else None, _ptr(out) if which == "lag" else None, qa.mem))
    return _shape_out(out, qa.single)


def keC(s: System, c: Config):
    """keC (Hamilton.hs:288-296)."""
    return _observe_config(s, c, "ke")


def lagrangian(s: System, c: Config):
    """lagrangian (Hamilton.hs:301-309)."""
    return _observe_config(s, c, "lag")


def hamEqs(s: System, ph: Phase):
    """hamEqs (Hamilton.hs:370-387): returns (dH/dp, -dH/dq)."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    dq, dp, st = qa.like(s.n), qa.like(s.n), qa.like(None, "i4")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_hameqs_batch(s._h, qa.B, qa.ptr, pa.ptr, _ptr(dq), _ptr(dp), _ptr(st), qa.mem))
    s._after(st, qa.single, "hamEqs")
    return _shape_out(dq, qa.single), _shape_out(dp, qa.single)


def sampleConfig(s: System, q_box, qd_box, start: int, count: int, seed: int, device=None) -> Config:
    """Initial Configs of trajectories start .. start + count - 1 of an ensemble, drawn ON THE DEVICE from the global index
    (hamk_sample_batch): uniform boxes q_box / qd_box = n pairs (lo, hi).  Same bits as
    `examples.sample_config` for any (start, count): shards need no host array and no scatter.  device: a torch CUDA
    device (tensors stay in HBM) or None (numpy arrays through the host-staged path)."""
    n = s.n
    if len(q_box) != n or len(qd_box) != n:
        raise ValueError(f"boxes must have {n} (lo, hi) pairs")
    arr = lambda xs: (ctypes.c_double * n)(*[float(x) for x in xs])
    qlo, qhi = arr([b[0] for b in q_box]), arr([b[1] for b in q_box])
    dlo, dhi = arr([b[0] for b in qd_box]), arr([b[1] for b in qd_box])
    if device is not None:
        dev = torch.device(device)
        q = torch.empty((n, int(count)), dtype=torch.float64, device=dev)
        qd = torch.empty_like(q)
    else:
        q, qd = np.empty((n, int(count))), np.empty((n, int(count)))
    qa = _Arr(q, n, "positions")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_sample_batch(s._h, int(count), int(start), int(seed), qlo, qhi, dlo, dhi, _ptr(q), _ptr(qd), qa.mem))
    return Config(q, qd)


# ---------------------------------------------------------------------------------------
# time stepping
# ---------------------------------------------------------------------------------------
def stepHam(r: float, s: System, ph: Phase, inplace: bool = False) -> Phase:
    """stepHam (Hamilton.hs:390-402): adaptive RKF45 (GSL semantics) from 0 to r.  inplace=True
    advances the given arrays without copying (ensemble loops; the reference's signature is pure)."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    st, ns = qa.like(None, "i4"), qa.like(None, "i4")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_step_ham_batch(s._h, qa.B, _ptr(q), _ptr(p), float(r), _ptr(st), _ptr(ns), qa.mem))
    s.last_nsub = ns
    s._after(st, qa.single, "stepHam")
    return Phase(_shape_out(q, qa.single), _shape_out(p, qa.single))


def iterateStepHam(r: float, ncalls: int, s: System, ph: Phase, every: int = 0, inplace: bool = False):
    """`iterate (stepHam r s)` (README.md:150; the demo's frame loop, app/Examples.hs:429) -- `ncalls` consecutive
    stepHam r in ONE launch (hamk_step_ham_iterate): bit-identical to calling stepHam `ncalls` times, without
    the launch and synchronisation per call.  Returns the final Phase, or (final Phase, frames) when
    every > 0: frames = the Phase after every `every`-th call, arrays shaped [ncalls // every, n(, B)]."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    st, ns = qa.like(None, "i4"), qa.like(None, "i4")
    rows = (int(ncalls) // int(every)) if every > 0 else 0
    fq = qa.like(s.n, lead=(rows,)) if rows else None
    fp = qa.like(s.n, lead=(rows,)) if rows else None
    with s._on(qa):
        _abi.check(_abi.lib().hamk_step_ham_iterate(s._h, qa.B, _ptr(q), _ptr(p), float(r), int(ncalls), int(every) if rows else 0,
                                                    _ptr(fq), _ptr(fp), _ptr(st), _ptr(ns), qa.mem))
    s.last_nsub = ns
    s._after(st, qa.single, "iterateStepHam")
    out = Phase(_shape_out(q, qa.single), _shape_out(p, qa.single))
    if every > 0:
        if rows == 0:
            return out, Phase(np.empty((0, s.n)), np.empty((0, s.n)))
        return out, Phase(_shape_out(fq, qa.single), _shape_out(fp, qa.single))
    return out


def evolveHam(s: System, p0: Phase, ts, h0: float = 0.0, eps_abs: float = 0.0, eps_rel: float = 0.0) -> List[Phase]:
    """evolveHam (Hamilton.hs:433-462): the state at each of the >= 2 times; element 0 is p0."""
    ts = np.ascontiguousarray(np.asarray(ts, dtype=np.float64))
    if ts.ndim != 1 or len(ts) < 2:
        raise ValueError("evolveHam needs at least two solution times (2 <= s)")
    qa, pa = _pair(p0.positions, "positions", p0.momenta, "momenta", s.n)
    nt = len(ts)
    qo, po = qa.like(s.n, lead=(nt,)), qa.like(s.n, lead=(nt,))
    st, ns = qa.like(None, "i4"), qa.like(None, "i4")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_evolve_ham_batch(
            s._h, qa.B, qa.ptr, pa.ptr, nt, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _ptr(qo), _ptr(po),
            float(h0), float(eps_abs), float(eps_rel), _ptr(st), _ptr(ns), qa.mem))
    s.last_nsub = ns
    s._after(st, qa.single, "evolveHam")
    return [Phase(_shape_out(qo[r], qa.single), _shape_out(po[r], qa.single)) for r in range(nt)]


def evolveHam_(s: System, p0: Phase, ts: Sequence[float]) -> List[Phase]:
    """evolveHam' (Hamilton.hs:409-429): [] -> []; [x] -> evolve over [0, x] and drop the first."""
    ts = list(ts)
    if not ts:
        return []
    if len(ts) == 1:
        return evolveHam(s, p0, [0.0, ts[0]])[1:]
    return evolveHam(s, p0, ts)


def stepHamC(r: float, s: System, c: Config) -> Config:
    """stepHamC (Hamilton.hs:502-515)."""
    return fromPhase(s, stepHam(r, s, toPhase(s, c)))


def evolveHamC(s: System, c0: Config, ts) -> List[Config]:
    """evolveHamC (Hamilton.hs:486-500)."""
    return [fromPhase(s, ph) for ph in evolveHam(s, toPhase(s, c0), ts)]


def evolveHamC_(s: System, c0: Config, ts: Sequence[float]) -> List[Config]:
    """evolveHamC' (Hamilton.hs:470-484)."""
    return [fromPhase(s, ph) for ph in evolveHam_(s, toPhase(s, c0), ts)]


def rk4Steps(dt: float, nsteps: int, s: System, ph: Phase, inplace: bool = False, drift_tol: float = 0.0) -> Phase:
    """Classic fixed-step RK4 over hamEqs -- named by BASELINE.json's north_star; the
    reference has no fixed-step integrator.  inplace=True advances the
    given device/host arrays without copying (bench path).  drift_tol > 0: the launch
    checks its own energy invariant and sets ST_DRIFT in `System.last_status` where
    |H_exit - H_entry| > drift_tol * max(1, |H_entry|) (hamk_rk4_steps_checked)."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    st = qa.like(None, "i4")
    with s._on(qa):
        _abi.check(_abi.lib().hamk_rk4_steps_checked(s._h, qa.B, _ptr(q), _ptr(p), float(dt), int(nsteps), float(drift_tol),
                                                     _ptr(st), qa.mem))
    s.last_status = st
    return Phase(_shape_out(q, qa.single), _shape_out(p, qa.single))


def symplecticSteps(dt: float, nsteps: int, s: System, ph: Phase, order: int = 2, iters: int = 0, inplace: bool = False,
                    with_residual: bool = False):
    """Symplectic fixed-step stepping (hamk_symplectic_steps; no reference counterpart): `nsteps` steps of `dt` by the
    implicit midpoint rule (order=2) or its three-substep symmetric composition (order=4), every substep solved by
    `iters` fixed-point iterations (1..64; 0 = the library's 8) -- a fixed count, so cost and bits do not depend on
    convergence.  One trajectory per lane: n <= 16.  with_residual=True returns (Phase, residual): per trajectory the
    largest last-iteration update, the way to learn that `iters` was too small for this dt."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    # zeroed: with nothing to do (nsteps = 0, an empty ensemble) the call returns HAMK_OK without writing status / residual
    st = qa.like(None, "i4", zero=True)
    res = qa.like(None, zero=True) if with_residual else None
    with s._on(qa):
        _abi.check(_abi.lib().hamk_symplectic_steps(s._h, qa.B, _ptr(q), _ptr(p), float(dt), int(nsteps), int(order), int(iters),
                                                    _ptr(res), _ptr(st), qa.mem))
    s._after(st, qa.single, "symplecticSteps")
    out = Phase(_shape_out(q, qa.single), _shape_out(p, qa.single))
    return (out, _shape_out(res, qa.single)) if with_residual else out


def lyapunovSteps(dt: float, nintervals: int, every: int, s: System, ph: Phase, w: Optional[Phase] = None, d0: float = 1e-7,
                  logsum=None, inplace: bool = False):
    """Largest-Lyapunov-exponent stepping fused with RK4 (hamk_lyapunov_steps; no reference counterpart; Benettin's
    two-trajectory method): `nintervals` intervals of `every` RK4 steps of `dt`, the shadow trajectory y + d0 w renormalised
    after each.  Returns (Phase, w, logsum): the new state, the new deviation as a Phase-shaped pair (its `positions` /
    `momenta` are wq / wp) and the running sum of log(d / d0); the exponent estimate is logsum / (nintervals * every * dt).
    w=None: every component 1 / sqrt(2n); a given w is used as it is (a unit vector is the caller's business).
    logsum=None: zeros.  Feeding the returned w and logsum to the next call continues the run bit for bit.  inplace=True
    advances the given arrays (state, and w / logsum where given) without copying.  One trajectory per lane: n <= 16."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    if w is None:
        wq, wp = qa.like(s.n), qa.like(s.n)
        wq[...] = 1.0 / np.sqrt(2.0 * s.n); wp[...] = 1.0 / np.sqrt(2.0 * s.n)
    else:
        wqa, wpa = _pair(w.positions, "w.positions", w.momenta, "w.momenta", s.n)
        if wqa.B != qa.B or wqa.device != qa.device or (qa.device and wqa.a.device != qa.a.device):
            raise ValueError("w must describe the ensemble of the state, in the same memory")
        if inplace:
            _in_place(wqa, w.positions, "w.positions"); _in_place(wpa, w.momenta, "w.momenta")
        wq, wp = (wqa.a, wpa.a) if inplace else (wqa.clone(), wpa.clone())
    if logsum is None:
        ls = qa.like(None, zero=True)
    else:
        la = _Arr(logsum.reshape(1, -1) if _is_torch(logsum) else np.asarray(logsum, dtype=np.float64).reshape(1, -1), 1, "logsum")
        if la.B != qa.B or la.device != qa.device or (qa.device and la.a.device != qa.a.device):
            raise ValueError(f"logsum: expected {qa.B} values in the memory of the state")
        if inplace:
            _in_place(la, logsum, "logsum")
        ls = (la.a if inplace else la.clone()).reshape(qa.B)
    # zeroed: with nothing to do (nintervals = 0, an empty ensemble) the call returns HAMK_OK without writing status
    st = qa.like(None, "i4", zero=True)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_lyapunov_steps(s._h, qa.B, _ptr(q), _ptr(p), _ptr(wq), _ptr(wp), float(dt), int(nintervals), int(every),
                                                  float(d0), _ptr(ls), _ptr(st), qa.mem))
    s._after(st, qa.single, "lyapunovSteps")
    return (Phase(_shape_out(q, qa.single), _shape_out(p, qa.single)), Phase(_shape_out(wq, qa.single), _shape_out(wp, qa.single)),
            _shape_out(ls, qa.single))


class Hits:
    """What poincareSteps recorded: `positions`, `momenta` [max_hits, n, B] (row r: the state at a trajectory's r-th crossing),
    `times` [max_hits, B] (in units of dt: steps taken + the fraction of the crossing step) and `count` [B] (int32; crossings seen,
    which may exceed max_hits -- rows at or beyond min(count, max_hits) hold nothing).  For one trajectory the B axis is dropped."""

    def __init__(self, positions, momenta, times, count):
        self.positions = positions
        self.momenta = momenta
        self.times = times
        self.count = count

    def __repr__(self):
        return f"Hits {{count = {self.count!r}, max_hits = {self.positions.shape[0]}}}"


def poincareSteps(dt: float, nsteps: int, s: System, ph: Phase, coord: int, level: float = 0.0, period: float = 0.0, direction: int = 1,
                  max_hits: int = 16, hits: Optional[Hits] = None, step0: int = 0, inplace: bool = False):
    """Poincare sections fused with RK4 (hamk_poincare_steps; no reference counterpart): `nsteps` RK4 steps of `dt`, and the
    crossings of component `coord` of [q; p] (coord < n: positions, else momenta) through y = level (period = 0) or
    y = level mod period, located inside the step on RK4's cubic continuous extension and recorded inside the launch.
    direction: +1 upward crossings, -1 downward, 0 both; at most one per step.  Returns (Phase, Hits).  hits=None: zeroed buffers
    of `max_hits` rows; passing the returned Hits back with step0 = the steps taken so far continues the run bit for bit (its row
    count then replaces max_hits).  Hits.count keeps counting beyond the rows there are.  inplace=True advances the given arrays
    (state, and the hit buffers where given) without copying.  One trajectory per lane: n <= 16."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    if hits is None:
        rows = int(max_hits)
        if rows < 1:
            raise ValueError("max_hits must be at least 1")
        hq, hp = qa.like(s.n, lead=(rows,), zero=True), qa.like(s.n, lead=(rows,), zero=True)
        ht, hn = qa.like(None, lead=(rows,), zero=True), qa.like(None, "i4", zero=True)
    else:
        rows = int(hits.positions.shape[0])
        bufs = []
        for a, shape, name, f8 in ((hits.positions, (rows, s.n, qa.B), "hits.positions", True), (hits.momenta, (rows, s.n, qa.B), "hits.momenta", True),
                                   (hits.times, (rows, qa.B), "hits.times", True), (hits.count, (qa.B,), "hits.count", False)):
            if _is_torch(a) != qa.device or (qa.device and a.device != qa.a.device):
                raise ValueError(f"{name} must live in the memory of the state")
            if not qa.device:
                a = np.asarray(a)
            want = torch.float64 if (f8 and qa.device) else torch.int32 if qa.device else np.float64 if f8 else np.int32
            if a.dtype != want or int(np.prod(a.shape)) != int(np.prod(shape)):
                raise ValueError(f"{name}: expected {'float64' if f8 else 'int32'} of shape {shape}")
            b = a.reshape(shape)
            if qa.device:
                b = b.contiguous()
                same = b.data_ptr() == a.data_ptr()
                b = b if inplace else b.clone()
            else:
                b = np.ascontiguousarray(b)
                same = b.ctypes.data == a.ctypes.data
                b = b if inplace else b.copy()
            if inplace and not same:
                raise ValueError(f"inplace=True needs {name} contiguous")
            bufs.append(b)
        hq, hp, ht, hn = bufs
    # zeroed: with nothing to do (nsteps = 0, an empty ensemble) the call returns HAMK_OK without writing status
    st = qa.like(None, "i4", zero=True)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_poincare_steps(s._h, qa.B, _ptr(q), _ptr(p), float(dt), int(nsteps), int(coord), float(level), float(period),
                                                  int(direction), rows, _ptr(hq), _ptr(hp), _ptr(ht), _ptr(hn), int(step0), _ptr(st), qa.mem))
    s._after(st, qa.single, "poincareSteps")
    drop = (lambda x: x[..., 0]) if qa.single else (lambda x: x)
    return Phase(_shape_out(q, qa.single), _shape_out(p, qa.single)), Hits(drop(hq), drop(hp), drop(ht), drop(hn))


class Exits:
    """What exitSteps keeps per trajectory: `code` [B] (int32: -1 still running, 2 g + side stopped by gate g through its lower /
    upper bound, -2 stopped because the state stopped being finite), `t` [B] (the exit time in units of dt: steps taken + the
    fraction of the exit step) and `q`, `p` [n, B] (the state at the exit).  Entries of running trajectories hold what they held at
    entry (zero for a new run).  For one trajectory the B axis is dropped."""

    def __init__(self, code, t, q, p):
        self.code = code
        self.t = t
        self.q = q
        self.p = p

    def __repr__(self):
        return f"Exits {{code = {self.code!r}, t = {self.t!r}}}"


def _gate_array(gates):
    """[(coord, lo, hi), ...] -> a ctypes array of hamk_gate (host memory, as the ABI wants it)."""
    gates = list(gates)
    arr = (_abi.hamk_gate * max(1, len(gates)))()
    for g, (coord, lo, hi) in enumerate(gates):
        arr[g].coord, arr[g].reserved, arr[g].lo, arr[g].hi = int(coord), 0, float(lo), float(hi)
    return arr, len(gates)


def exitSteps(dt: float, nsteps: int, s: System, ph: Phase, gates, exits: Optional[Exits] = None, step0: int = 0, inplace: bool = False):
    """First-exit times fused with RK4 (hamk_exit_steps; no reference counterpart): up to `nsteps` RK4 steps of `dt`; after every
    step a trajectory whose state has left a gate stops -- `gates`: 1 to 4 tuples (coord, lo, hi), component `coord` of [q; p]
    (coord < n: positions, else momenta) must stay in [lo, hi], either bound may be infinite -- and a wavefront whose trajectories
    have all stopped ends its stepping.  Returns (Phase, Exits): a stopped trajectory's state is the END of its exit step,
    Exits.q / .p the state at the exit, located inside the step on RK4's cubic continuous extension.  exits=None: a new run (every
    code -1); passing the returned Exits back with step0 = the steps taken so far continues the run bit for bit.  inplace=True
    advances the given arrays (state, and the Exits where given) without copying.  One trajectory per lane: n <= 16."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    if exits is None:
        code, te = qa.like(None, "i4", zero=True), qa.like(None, zero=True)
        code -= 1
        eq, ep = qa.like(s.n, zero=True), qa.like(s.n, zero=True)
    else:
        bufs = []
        for a, shape, name, f8 in ((exits.code, (qa.B,), "exits.code", False), (exits.t, (qa.B,), "exits.t", True),
                                   (exits.q, (s.n, qa.B), "exits.q", True), (exits.p, (s.n, qa.B), "exits.p", True)):
            if _is_torch(a) != qa.device or (qa.device and a.device != qa.a.device):
                raise ValueError(f"{name} must live in the memory of the state")
            if not qa.device:
                a = np.asarray(a)
            want = torch.float64 if (f8 and qa.device) else torch.int32 if qa.device else np.float64 if f8 else np.int32
            if a.dtype != want or int(np.prod(a.shape)) != int(np.prod(shape)):
                raise ValueError(f"{name}: expected {'float64' if f8 else 'int32'} of shape {shape}")
            b = a.reshape(shape)
            if qa.device:
                b = b.contiguous()
                same = b.data_ptr() == a.data_ptr()
                b = b if inplace else b.clone()
            else:
                b = np.ascontiguousarray(b)
                same = b.ctypes.data == a.ctypes.data
                b = b if inplace else b.copy()
            if inplace and not same:
                raise ValueError(f"inplace=True needs {name} contiguous")
            bufs.append(b)
        code, te, eq, ep = bufs
    garr, ngates = _gate_array(gates)
    # zeroed: with nothing to do (nsteps = 0, an empty ensemble) the call returns HAMK_OK without writing status
    st = qa.like(None, "i4", zero=True)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_exit_steps(s._h, qa.B, _ptr(q), _ptr(p), float(dt), int(nsteps), ctypes.addressof(garr), ngates, _ptr(code), _ptr(te),
                                              _ptr(eq), _ptr(ep), int(step0), _ptr(st), qa.mem))
    s._after(st, qa.single, "exitSteps")
    drop = (lambda x: x[..., 0]) if qa.single else (lambda x: x)
    return Phase(_shape_out(q, qa.single), _shape_out(p, qa.single)), Exits(drop(code), drop(te), drop(eq), drop(ep))


class Record:
    """What recordSteps recorded: `positions`, `momenta` [max_rows, n, B] or None (row k: the state after k * every steps, row 0
    the initial state), `energy` [max_rows, B] or None (the Hamiltonian of that state) and `rows`: how many rows of the run are
    filled so far -- rows at or beyond it hold nothing.  For one trajectory the B axis is dropped."""

    def __init__(self, positions, momenta, energy, rows):
        self.positions = positions
        self.momenta = momenta
        self.energy = energy
        self.rows = rows

    def __repr__(self):
        have = self.positions if self.positions is not None else self.energy
        return f"Record {{rows = {self.rows}, max_rows = {have.shape[0]}}}"


def recordSteps(dt: float, nsteps: int, every: int, s: System, ph: Phase, max_rows: Optional[int] = None, states: bool = True,
                energy: bool = False, record: Optional[Record] = None, step0: int = 0, inplace: bool = False):
    """Trajectory recording fused with RK4 (hamk_record_steps; evolveHam's rows on a fixed step): `nsteps` RK4 steps of `dt`, and
    the state (states=True) and / or its Hamiltonian (energy=True) after every `every`-th step of the run written to row buffers
    inside the launch; row 0 is the initial state.  Returns (Phase, Record).  record=None: a new run with buffers of `max_rows` rows
    (None: exactly the rows the run fills, (step0 + nsteps) // every + 1); rows beyond max_rows are dropped.  Passing the returned
    Record back with step0 = the steps taken so far continues the run bit for bit (its buffers then say what is recorded and how
    many rows there are).  inplace=True advances the given arrays (state, and the Record's buffers where given) without copying.
    One trajectory per lane: n <= 16."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", s.n)
    if inplace:
        _in_place(qa, ph.positions, "positions"); _in_place(pa, ph.momenta, "momenta")
    q, p = (qa.a, pa.a) if inplace else (qa.clone(), pa.clone())
    if int(every) < 1:
        raise ValueError("every must be at least 1")
    if record is None:
        rows = (int(step0) + int(nsteps)) // int(every) + 1 if max_rows is None else int(max_rows)
        if rows < 1:
            raise ValueError("max_rows must be at least 1")
        if not states and not energy:
            raise ValueError("nothing to record: states and energy are both off")
        rq = qa.like(s.n, lead=(rows,), zero=True) if states else None
        rp = qa.like(s.n, lead=(rows,), zero=True) if states else None
        rh = qa.like(None, lead=(rows,), zero=True) if energy else None
        before = 0
    else:
        have = record.positions if record.positions is not None else record.energy
        if have is None or (record.positions is None) != (record.momenta is None):
            raise ValueError("record: positions and momenta go together, and at least one of them and energy must be there")
        rows = int(have.shape[0])
        bufs = []
        for a, shape, name in ((record.positions, (rows, s.n, qa.B), "record.positions"), (record.momenta, (rows, s.n, qa.B), "record.momenta"),
                               (record.energy, (rows, qa.B), "record.energy")):
            if a is None:
                bufs.append(None)
                continue
            if _is_torch(a) != qa.device or (qa.device and a.device != qa.a.device):
                raise ValueError(f"{name} must live in the memory of the state")
            if not qa.device:
                a = np.asarray(a)
            if a.dtype != (torch.float64 if qa.device else np.float64) or int(np.prod(a.shape)) != int(np.prod(shape)):
                raise ValueError(f"{name}: expected float64 of shape {shape}")
            b = a.reshape(shape)
            if qa.device:
                b = b.contiguous()
                same = b.data_ptr() == a.data_ptr()
                b = b if inplace else b.clone()
            else:
                b = np.ascontiguousarray(b)
                same = b.ctypes.data == a.ctypes.data
                b = b if inplace else b.copy()
            if inplace and not same:
                raise ValueError(f"inplace=True needs {name} contiguous")
            bufs.append(b)
        rq, rp, rh = bufs
        before = int(record.rows)
    # zeroed: with nothing to do (nsteps = 0, an empty ensemble) the call returns HAMK_OK without writing status or any row
    st = qa.like(None, "i4", zero=True)
    with s._on(qa):
        _abi.check(_abi.lib().hamk_record_steps(s._h, qa.B, _ptr(q), _ptr(p), float(dt), int(nsteps), int(every), rows, _ptr(rq), _ptr(rp), _ptr(rh),
                                                int(step0), _ptr(st), qa.mem))
    s._after(st, qa.single, "recordSteps")
    filled = min(rows, (int(step0) + int(nsteps)) // int(every) + 1) if (int(nsteps) > 0 and qa.B > 0) else before
    drop = (lambda x: None if x is None else x[..., 0]) if qa.single else (lambda x: x)
    return Phase(_shape_out(q, qa.single), _shape_out(p, qa.single)), Record(drop(rq), drop(rp), drop(rh), filled)


# ---------------------------------------------------------------------------------------
# ensemble checkpoint: device- or host-resident state <-> one flat file
# ---------------------------------------------------------------------------------------
def saveCheckpoint(path: str, ph: Phase, n: int, steps_done: int = 0, seed: int = 0, t: float = 0.0) -> None:
    """hamk_checkpoint_write: q[n][B], p[n][B] (numpy or torch CUDA tensors) + bookkeeping."""
    qa, pa = _pair(ph.positions, "positions", ph.momenta, "momenta", n)
    if qa.device:
        torch.cuda.current_stream(qa.a.device).synchronize()     # the copy out runs on the null stream
    ctx = torch.cuda.device(qa.a.device) if qa.device else contextlib.nullcontext()
    with ctx:
        _abi.check(_abi.lib().hamk_checkpoint_write(str(path).encode(), n, qa.B, qa.ptr, pa.ptr, qa.mem,
                                                    int(steps_done), int(seed), float(t)))


def checkpointInfo(path: str) -> dict:
    n, B, st, seed, t = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_double()
    _abi.check(_abi.lib().hamk_checkpoint_info(str(path).encode(), ctypes.byref(n), ctypes.byref(B), ctypes.byref(st),
                                               ctypes.byref(seed), ctypes.byref(t)))
    return {"n": n.value, "B": B.value, "steps_done": st.value, "seed": seed.value, "t": t.value}


def loadCheckpoint(path: str, device=None):
    """Returns (Phase, info).  device=None: numpy arrays; a torch device: CUDA tensors on it."""
    info = checkpointInfo(path)
    n, B = info["n"], info["B"]
    if device is None:
        q, p = np.empty((n, B)), np.empty((n, B))
        _abi.check(_abi.lib().hamk_checkpoint_read(str(path).encode(), n, B, q.ctypes.data, p.ctypes.data, MEM_HOST))
    else:
        dev = torch.device(device)
        q = torch.empty((n, B), dtype=torch.float64, device=dev)
        p = torch.empty((n, B), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _abi.check(_abi.lib().hamk_checkpoint_read(str(path).encode(), n, B, q.data_ptr(), p.data_ptr(), MEM_DEVICE))
    return Phase(q, p), info
