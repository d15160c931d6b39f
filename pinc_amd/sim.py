"""Python handle on one rank of the MI355X PINC simulation (libpinc.so).

This mirrors the reference's run mode regular() (src/main.c:50-304): the
ini file plus ``key=value`` overrides select the operators, normalise the
units and size the population and grids; ``init()`` builds the initial state
and ``step()`` runs one timestep on the GPU.  All computation happens in the
native library; this wrapper only moves arguments and diagnostics.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import HOST, PincSimOpts


class Sim:
    def __init__(self, ini: str, overrides: Sequence[str] = (), *, literal: bool = False,
                 perturb: bool = True, maxwell: bool = False, device_init: bool = False,
                 seed: int = 0, rank: int = 0, nranks: int = 1, device: int = 0,
                 comm_id: bytes | None = None, timing: bool = False, transport=None):
        """transport: a pinc_amd.transport.GlooTransport for multi-rank runs
        without RCCL (several ranks on one GPU, tests); default RCCL."""
        self._id_buf = None
        self._transport = transport
        HOST.pinc_set_host_transport(C.byref(transport.struct) if transport is not None else None)
        opts = PincSimOpts()
        opts.literal = int(literal)
        opts.perturb = int(perturb)
        opts.maxwell = int(maxwell)
        opts.deviceInit = int(device_init)
        opts.seed = seed
        opts.rank = rank
        opts.nranks = nranks
        opts.device = device
        opts.timing = int(timing)
        if comm_id is not None:
            self._id_buf = (C.c_ubyte * len(comm_id)).from_buffer_copy(comm_id)
            opts.commId = C.cast(self._id_buf, C.c_void_p)
        arr = (C.c_char_p * max(1, len(overrides)))(*[o.encode() for o in overrides])
        self._h = HOST.pinc_sim_create(str(ini).encode(), len(overrides), arr, C.byref(opts))
        if not self._h:
            raise RuntimeError("pinc_sim_create failed: " + HOST.pinc_last_error().decode())
        self.nspecies = HOST.pinc_sim_nspecies(self._h)
        self.ndims = HOST.pinc_sim_ndims(self._h)

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            HOST.pinc_sim_free(self._h)
            self._h = None
            if self._transport is not None:
                HOST.pinc_set_host_transport(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def init(self) -> None:
        HOST.pinc_sim_init(self._h)

    def step(self, n: int = 1) -> None:
        """n iterations of the main loop (one library call: no return to
        Python between them)."""
        if n == 1:
            HOST.pinc_sim_step(self._h)
        elif n > 1:
            HOST.pinc_sim_steps(self._h, n)

    def op(self, name: str) -> None:
        if HOST.pinc_sim_op(self._h, name.encode()):
            raise ValueError(f"unknown op {name}")

    def sync(self) -> None:
        HOST.pinc_sim_sync(self._h)

    # -- output (the reference's .h5 files) ---------------------------------
    def open_output(self) -> None:
        """pop/rho/phi/E/history files under files:output (main.c:118-131)."""
        HOST.pinc_sim_open_output(self._h)

    def write_output(self, n: float) -> None:
        """main.c:262-266 for step n: E, rho, phi at n, positions at n,
        velocities at n + 0.5, energy rows."""
        HOST.pinc_sim_write_output(self._h, float(n))

    # -- diagnostics -------------------------------------------------------
    def energy(self) -> tuple[float, float, np.ndarray]:
        ke, pe = C.c_double(), C.c_double()
        kes = (C.c_double * self.nspecies)()
        HOST.pinc_sim_energy(self._h, C.byref(ke), C.byref(pe), kes)
        return ke.value, pe.value, np.array(kes)

    @property
    def cycles(self) -> int:
        return HOST.pinc_sim_cycles(self._h)

    def mg_limit(self, max_cycles: int = 0, hist_cap: int = 0) -> None:
        """Cap the V-cycles of one multigrid solve (0: until converged) and
        record up to hist_cap per-cycle RMS residuals (mgSetLimit)."""
        if HOST.pinc_sim_mg_limit(self._h, max_cycles, hist_cap):
            raise RuntimeError("mg_limit: the Poisson solver is not multigrid")

    @property
    def mg_levels(self) -> int:
        """Levels of the multigrid hierarchy in use (0 for the spectral solver)."""
        return HOST.pinc_sim_mg_levels(self._h)

    @property
    def mg_shard(self) -> int:
        """Halo planes of the sharded multigrid level 0 (0: replicated solve)."""
        return HOST.pinc_sim_mg_shard(self._h)

    @property
    def spectral_distributed(self) -> bool:
        """The spectral solve is slab-distributed (no gather of rho)."""
        return bool(HOST.pinc_sim_spectral_distributed(self._h))

    @property
    def obj_collected(self) -> float:
        """Charge the immersed objects collected since init (0 without objects)."""
        return HOST.pinc_sim_obj_collected(self._h)

    def mg_history(self) -> np.ndarray:
        """RMS residual after each V-cycle of the last solve (mgHistory)."""
        n = HOST.pinc_sim_mg_history(self._h, None, 0)
        out = np.zeros(max(n, 0))
        if n > 0:
            HOST.pinc_sim_mg_history(self._h, out.ctypes.data, n)
        return out

    def count(self, s: int) -> int:
        return HOST.pinc_sim_pop_count(self._h, s)

    def total_particles(self) -> int:
        return HOST.pinc_sim_total_particles(self._h)

    def particles(self, s: int) -> tuple[np.ndarray, np.ndarray]:
        n = self.count(s)
        pos = np.zeros((n, self.ndims))
        vel = np.zeros((n, self.ndims))
        HOST.pinc_sim_pop_get(self._h, s, pos.ctypes.data, vel.ctypes.data)
        return pos, vel

    def set_particles(self, s: int, pos: np.ndarray, vel: np.ndarray) -> None:
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        vel = np.ascontiguousarray(vel, dtype=np.float64)
        if HOST.pinc_sim_pop_set(self._h, s, pos.shape[0], pos.ctypes.data, vel.ctypes.data):
            raise RuntimeError("pinc_sim_pop_set failed")

    def grid_shape(self, which: int) -> tuple[int, ...]:
        size = (C.c_int * 4)()
        HOST.pinc_sim_grid_shape(self._h, which, size)
        return tuple(size)

    def grid(self, which: int) -> np.ndarray:
        """rho (0), phi (1) or E (2) in the reference layout (value-major,
        ghost layers included), shaped [nz+2, ny+2, nx+2, nValues] for 3-D."""
        size = self.grid_shape(which)
        rank = self.ndims + 1
        out = np.zeros(int(np.prod(size[:rank])))
        HOST.pinc_sim_grid_get(self._h, which, out.ctypes.data)
        return out.reshape(tuple(reversed(size[:rank])))

    def set_grid(self, which: int, values: np.ndarray) -> None:
        v = np.ascontiguousarray(values, dtype=np.float64).ravel()
        HOST.pinc_sim_grid_set(self._h, which, v.ctypes.data)

    def moments(self, s: int) -> np.ndarray:
        """The first velocity moments of species s on this rank's true nodes,
        halo folded: shape true nodes + (NM,), [nz, ny, nx, 10] in 3-D (NM =
        1 + nd + nd (nd + 1) / 2).  Per node the CIC-weighted sums of 1, v_i
        and v_i v_j (i <= j: xx xy xz yy yz zz) over the species' particles
        at (x_n, v_n+1/2), in code units; pinc_amd.moments.derive turns them
        into density, bulk velocity, pressure and temperature."""
        size = (C.c_int * 4)()
        n = HOST.pinc_sim_moments_shape(self._h, size)
        out = np.zeros(n)
        if HOST.pinc_sim_moments(self._h, s, out.ctypes.data):
            raise ValueError(f"moments: no species {s}")
        return out.reshape(tuple(reversed(size[1:1 + self.ndims])) + (size[0],))

    def phase_space(self, s: int, axes=("x", "vx"), bins=(64, 64), lo=(0.0, -1.0), hi=(1.0, 1.0)):
        """Histogram of species s over one or two of x y z vx vy vz at
        (x_n, v_n+1/2): bins[a] equal bins over [lo[a], hi[a]), positions in
        the global frame (particles() + offset), velocities in code units;
        the binning rule is pinc_hip_phase_hist's.  Returns (hist,
        outside): float64 counts of shape [bins[1], bins[0]] ([bins[0]] for
        one axis), summed over the ranks (the call is collective), and the
        number of particles outside the range."""
        from .phase import AXES
        axes = (axes,) if isinstance(axes, str) else tuple(axes)
        bins, lo, hi = (tuple(np.atleast_1d(a).tolist()) for a in (bins, lo, hi))
        na = len(axes)
        if na not in (1, 2) or any(a not in AXES for a in axes) or not (len(bins) == len(lo) == len(hi) == na):
            raise ValueError(f"phase_space: axes {axes} with bins {bins}, lo {lo}, hi {hi}")
        if any(int(b) != b or b < 1 for b in bins) or int(np.prod(bins)) > 1 << 24:
            raise ValueError(f"phase_space: bins {bins}")
        spec = _lib.PhaseSpec()
        spec.axis[1], spec.nbins[1] = -1, 1
        for a in range(na):
            spec.axis[a], spec.nbins[a], spec.lo[a], spec.hi[a] = AXES.index(axes[a]), int(bins[a]), lo[a], hi[a]
        out = np.zeros(tuple(int(b) for b in reversed(bins)))
        outside = C.c_double()
        if HOST.pinc_sim_phase_hist(self._h, s, C.byref(spec), out.ctypes.data, C.byref(outside)):
            raise ValueError(f"phase_space: bad species {s} or spec (axes {axes}, bins {bins}, lo {lo}, hi {hi})")
        return out, outside.value

    def collisions(self, s: int) -> tuple[int, int]:
        """(elastic, charge exchange): this rank's collisions of species s
        with the neutral background since the simulation was created (the
        ini's [collisions] section; zeros without one).  op("collide") runs
        one collision step on its own."""
        out = (C.c_ulonglong * 2)()
        if HOST.pinc_sim_collisions(self._h, s, out):
            raise ValueError(f"collisions: no species {s}")
        return int(out[0]), int(out[1])

    def ionizations(self, s: int) -> int:
        """This rank's electron-ion pairs born by the impact of species s on
        the neutral background since the simulation was created (the ini's
        collisions:ionNu, ionSigma, ionThreshold, ionSpecies; zero without
        them).  op("ionize") runs one ionisation step on its own."""
        out = C.c_ulonglong()
        if HOST.pinc_sim_ionizations(self._h, s, C.byref(out)):
            raise ValueError(f"ionizations: no species {s}")
        return int(out.value)

    def coulomb_count(self, a: int, b: int) -> int:
        """This rank's binary Coulomb collisions between species a and b since
        the simulation was created (the ini's collisions:coulombLog; zero
        without it).  op("coulomb") runs one step of them on its own."""
        out = C.c_ulonglong()
        if HOST.pinc_sim_coulomb_count(self._h, a, b, C.byref(out)):
            raise ValueError(f"coulomb_count: no species pair {a}, {b}")
        return int(out.value)

    def coulomb_coef(self, a: int, b: int) -> float:
        """K_ab of pinc_hip_coulomb for species a and b in the code's units
        (0 for a pair without a Coulomb logarithm)."""
        out = C.c_double()
        if HOST.pinc_sim_coulomb_coef(self._h, a, b, C.byref(out)):
            raise ValueError(f"coulomb_coef: no species pair {a}, {b}")
        return float(out.value)

    @property
    def offset(self) -> np.ndarray:
        """This rank's offset of the local frame (particles()) to the global
        one, per dimension."""
        off = (C.c_int * 3)()
        HOST.pinc_sim_offset(self._h, off)
        return np.array(off[:self.ndims], dtype=np.int64)

    def emigrants(self) -> np.ndarray:
        n = 3 ** self.ndims * self.nspecies
        out = np.zeros(n, dtype=np.int64)
        HOST.pinc_sim_emigrants(self._h, out.ctypes.data)
        return out.reshape(3 ** self.ndims, self.nspecies)

    def species(self) -> tuple[np.ndarray, np.ndarray]:
        q = np.zeros(self.nspecies)
        m = np.zeros(self.nspecies)
        HOST.pinc_sim_species(self._h, q.ctypes.data, m.ctypes.data)
        return q, m

    def timers(self) -> dict[str, float]:
        ms = np.zeros(_lib.NPHASES)
        HOST.pinc_sim_timers(self._h, ms.ctypes.data)
        return dict(zip(_lib.PHASES, ms.tolist()))

    def timers_reset(self) -> None:
        HOST.pinc_sim_timers_reset(self._h)


def h5_available() -> bool:
    return bool(HOST.pinc_h5_available())


def h5_read(path: str, name: str, attr: bool = False) -> np.ndarray:
    """A dataset (or double attribute) of an .h5 file, through the same
    run-time HDF5 binding the writer uses (h5py is not installed)."""
    if attr:
        out = np.zeros(1)
        n = HOST.pinc_h5_read(str(path).encode(), name.encode(), 1, out.ctypes.data, 1)
        if n < 0:
            raise KeyError(f"{path}: attribute {name}")
        return out
    dims = np.zeros(8, dtype=np.int64)
    r = HOST.pinc_h5_dims(str(path).encode(), name.encode(), dims.ctypes.data)
    if r < 0:
        raise KeyError(f"{path}: {name}")
    shape = tuple(int(d) for d in dims[:r])
    out = np.zeros(int(np.prod(shape)) if shape else 1)
    n = HOST.pinc_h5_read(str(path).encode(), name.encode(), 0, out.ctypes.data, out.size)
    if n < 0:
        raise KeyError(f"{path}: {name}")
    return out.reshape(shape)
