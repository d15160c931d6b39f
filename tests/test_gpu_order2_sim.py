"""methods:acc = puAccND2KE, methods:distr = puDistrND2 through Sim: the
selectors, the operators against the restatement tests/order2_ref.py, two
slabs against one, conservation, the Langmuir frequency, and no trace left in
a later order-1 run.

Bounds.  Deposit through the operator: the kernel bound (k + 8) eps
sum|terms| (tests/test_gpu_order2_kernel.py) with the terms scaled by |q_s|,
k summed over the species and over the planes the halo fold joins (each join
is one of the k - 1 additions).  The chain's gMul(q_0), gMul(1/q_1), gMul(q_1)
are exact for the configs' normalised charges -1 and +1.
Gather: the kernel's bound, on E as pinc_hip_field_chain rescales it for the
species (restated in float64 in the same order: bit-identical).
"""
import os
import socket
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import order2_ref as O
from pinc_amd import configs
from test_oracle_golden import ke_peak_omega

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EPS = O.EPS
S3 = (16, 16, 16)


def order2(cfg, thresholds="0.5"):
    cfg["methods"]["acc"] = "puAccND2KE"
    cfg["methods"]["distr"] = "puDistrND2"
    cfg["grid"]["thresholds"] = thresholds
    return cfg


def config(name):
    return configs.config(name, true_size=S3) if name == "cold3d" else configs.config(name)


def sim(cfg, **kw):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        return Sim(ini, **kw)
    finally:
        os.unlink(ini)


def check(rho, ref, what):
    err = np.abs(rho.astype(O.LD) - ref.M)
    lim = (ref.k + 8) * EPS * ref.A
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0.0))
    print(f"{what}: error / bound {worst:.3f}")
    assert np.all(err <= lim), (what, worst)
    return lim


@pytest.mark.parametrize("name", ["langmuir1d", "langmuir2d", "cold3d"])
def test_selectors_build_and_step(built, name):
    with sim(order2(config(name))) as s:
        s.init()
        n0 = s.total_particles()
        s.step(2)
        assert s.total_particles() == n0
        ke, pe, _ = s.energy()
        assert np.isfinite(ke) and np.isfinite(pe) and ke > 0


@pytest.mark.parametrize("name", ["langmuir1d", "langmuir2d", "cold3d"])
def test_thresholds_other_than_half_are_refused(built, name):
    """puSanity's message for order 2 (pusher.c:1074-1075) in pinc_last_error.
    msg(ERROR) exits the process (io.c:214-215), so the Sim is created in a
    child process, which reads pinc_last_error from an exit handler."""
    ini = configs.write_ini(order2(config(name), thresholds="0.1"))
    code = f"""import ctypes as C, sys
from pinc_amd import Sim, _lib
@C.CFUNCTYPE(None, C.c_int, C.c_void_p)
def report(status, arg):
    sys.stderr.write("pinc_last_error: " + _lib.HOST.pinc_last_error().decode() + "\\n")
    sys.stderr.flush()
C.CDLL(None).on_exit(report, None)
with Sim({str(ini)!r}) as s:
    s.init()
"""
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    finally:
        os.unlink(ini)
    assert r.returncode != 0
    assert "pinc_last_error: puAccND2KE requires grid:thresholds >=0.5\n" in r.stderr, r.stderr[-2000:]


def species_positions(n):
    return [O.particles(S3, n, 40 + sp) for sp in range(2)]


def test_deposit_and_gather_against_the_restatement(built):
    with sim(order2(config("cold3d"))) as s:
        s.init()
        q, m = s.species()
        rng = np.random.default_rng(9)
        pos = species_positions(3000)
        vel = [rng.uniform(-0.5, 0.5, size=p.shape) for p in pos]
        for sp in range(2):
            s.set_particles(sp, pos[sp], vel[sp])
        s.op("distr")
        rho = s.grid(0)
        assert rho.shape == (18, 18, 18, 1)
        refs = [O.folded(O.slab(O.deposit(pos[sp], S3), S3), S3[2]) for sp in range(2)]
        check(rho[1:-1, 1:-1, 1:-1, 0], O.charge_chain(refs, q), "rho after distr")

        # E on every node, the ghosts the periodic copies in every dimension
        Et = rng.uniform(-0.2, 0.2, size=(16, 16, 16, 3))
        E = np.pad(Et, ((1, 1), (1, 1), (1, 1), (0, 0)), mode="wrap")
        s.set_grid(2, E)
        s.op("acc")
        slabE = E[:, 1:-1, 1:-1, :]
        qm, mq = q / m, m / q
        for sp in range(2):
            Es = slabE * 1.0
            for t in range(sp):
                Es = (Es * qm[t]) * mq[t]
            Es = Es * qm[sp]
            dv, mag = O.gather(pos[sp], Es, S3)
            x, v = s.particles(sp)
            np.testing.assert_array_equal(x, pos[sp])
            err = np.abs(v.astype(O.LD) - (vel[sp].astype(O.LD) + dv))
            lim = (27 + 8) * EPS * mag + EPS * np.abs(v)
            print(f"species {sp}: velocity error / bound {float(np.max(err / lim)):.3f}")
            assert np.all(err <= lim)


def second_fold(pos):
    """one species' true nodes after main.c:226 and :232 on a deposit made
    without the literal factor: plain folded (ghost planes kept), plus the
    literal-2 weights, folded once more (test_order2_ref_cpu's
    test_literal_factors shows that this is literal 1 folded twice)"""
    plain, lit2 = (O.slab(O.deposit(pos, S3, literal), S3) for literal in (0, 2))

    def both(a, b):
        a = a.copy()
        a[S3[2]] += a[0]
        a[1] += a[S3[2] + 1]
        return O.fold(a + b, S3[2])
    return SimpleNamespace(M=both(plain.M, lit2.M), A=both(plain.A, lit2.A), k=both(plain.k, lit2.k))


def test_second_fold_against_the_restatement(built):
    """op fold_rho after op distr is main.c:232's second FROMHALO add on one
    order-2 deposit: pinc_literal_second_fold adds the literal-2 weights with
    the deposit's species chain, then the planes fold again.  The deposit's
    bound: the second fold's additions are among the k - 1 of its k terms, the
    literal factor (1, 3, 7, doubled) is the rounding the kernel bound counts."""
    with sim(order2(config("cold3d"))) as s:
        s.init()
        q, _ = s.species()
        pos = species_positions(3000)
        for sp in range(2):
            s.set_particles(sp, pos[sp], np.zeros_like(pos[sp]))
        s.op("distr")
        s.op("fold_rho")
        rho = s.grid(0)[1:-1, 1:-1, 1:-1, 0]
    ref = O.charge_chain([second_fold(p) for p in pos], q)
    assert np.any(ref.M != O.charge_chain([O.folded(O.slab(O.deposit(p, S3), S3), S3[2]) for p in pos], q).M)
    check(rho, ref, "rho after the second fold")


def _port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_two_slabs_equal_one(built, tmp_path):
    """rho of the same particles on two z-slabs of 8 planes and on one of 16,
    with particles planted within half a cell of both faces of each slab"""
    rng = np.random.default_rng(13)
    pos = species_positions(2000)
    for p in pos:
        face = np.array([0.5, 0.75, np.nextafter(8.5, 0.0), 8.25, 8.5, 8.75, np.nextafter(16.5, 0.0), 16.25, 16.0, 8.0,
                         1.0, 9.0])
        p[100:100 + len(face), 2] = face
        p[200:400, 2] = np.where(rng.random(200) < 0.5, 8.0, 16.0) + rng.uniform(-0.5, 0.5, 200)
        p[:, 2] = np.clip(p[:, 2], 0.5, np.nextafter(16.5, 0.0))
    with sim(order2(config("cold3d"))) as s:
        s.init()
        q, _ = s.species()
        off = s.offset.astype(np.float64)
        for sp in range(2):
            s.set_particles(sp, pos[sp], np.zeros_like(pos[sp]))
        s.op("distr")
        one = s.grid(0)[1:-1, 1:-1, 1:-1, 0]
    # the workers take the global frame, local + Sim.offset.  Both shifts are by
    # whole cells and exact in float64 (positions >= 0.5, offsets of at most 16),
    # so each rank deposits the coordinates of the one-slab run bit for bit,
    # minus its 8 planes
    parts = tmp_path / "parts.npz"
    np.savez(parts, pos0=pos[0] + off, pos1=pos[1] + off)
    cfg2 = order2(configs.config("cold3d", true_size=(16, 16, 8), nsub=(1, 1, 2)))
    cfg2["multigrid"]["mgLevels"] = "3"   # (8 planes per slab; the solver is not used here)
    ini2 = configs.write_ini(cfg2)
    out = tmp_path / "rho"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "order2_worker.py"),
           "--mode", "ranks", "--ini", ini2, "--out", str(out), "--particles", str(parts)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini2)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    two = np.concatenate([np.load(f"{out}_r{r}.npy") for r in range(2)], axis=0)
    ref = O.charge_chain([O.folded(O.slab(O.deposit(pos[sp], S3), S3), 16) for sp in range(2)], q)
    assert two.shape == one.shape == (16, 16, 16)
    lim = check(one, ref, "one slab")
    check(two, ref, "two slabs")
    worst = float(np.max(np.abs(two.astype(O.LD) - one) / lim))
    print(f"two slabs against one: difference / bound {worst:.3f}")
    assert np.all(np.abs(two.astype(O.LD) - one) <= lim)


def test_conservation_over_20_steps(built):
    with sim(order2(config("cold3d"))) as s:
        s.init()
        q, _ = s.species()
        counts = [s.count(sp) for sp in range(2)]
        for _ in range(20):
            s.step()      # (a set assert bit is a msg(ERROR): it ends the step and the process)
            assert [s.count(sp) for sp in range(2)] == counts
        s.op("distr")
        rho = s.grid(0)[1:-1, 1:-1, 1:-1, 0]
        n = sum(counts)
        scale = float(sum(abs(q[sp]) * counts[sp] for sp in range(2)))
        total = float(np.sum(rho.astype(O.LD)))
        want = float(sum(O.LD(q[sp]) * counts[sp] for sp in range(2)))
        print(f"sum rho {total!r}, sum q N {want!r}, bound {(n + 8) * EPS * scale:.3e}")
        assert abs(total - want) <= (n + 8) * EPS * scale


def _omega(cfg):
    ke = []
    with sim(cfg) as s:
        s.init()
        for _ in range(150):
            s.step()
            ke.append(s.energy()[0])
    return ke_peak_omega(np.array(ke), float(cfg["time"]["timeStep"]))


@pytest.mark.parametrize("name", ["langmuir1d", "langmuir2d"])
def test_langmuir_frequency_within_one_percent_of_order_1(built, name):
    om1 = _omega(config(name))
    om2 = _omega(order2(config(name)))
    print(f"{name}: omega order 1 {om1:.6f}, order 2 {om2:.6f}, ratio {om2 / om1:.5f}")
    assert abs(om2 - om1) <= 0.01 * om1, (om1, om2)


def test_no_effect_on_a_later_order_1_run(built, tmp_path):
    """after an order-2 Sim was used and closed, a default Sim in this
    process gives the energies of a fresh process.  Two runs add charge with
    float atomics in different orders, so equal means to 1e-11 relative (the
    bound derived in tests/test_gpu_moments_sim.py, ENERGY_RTOL)."""
    cfg = config("langmuir2d")
    ini = configs.write_ini(cfg)
    try:
        out = tmp_path / "fresh.npy"
        env = dict(os.environ, PYTHONPATH=str(ROOT))
        p = subprocess.run([sys.executable, str(ROOT / "tests" / "order2_worker.py"), "--mode", "energies", "--ini", ini,
                            "--out", str(out), "--steps", "3"], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        fresh = np.load(out)
        with sim(order2(config("langmuir2d"))) as s:
            s.init()
            s.step(3)
        rows = []
        with sim(cfg) as s:
            s.init()
            for _ in range(3):
                s.step()
                ke, pe, _ = s.energy()
                rows.append((ke, pe))
        np.testing.assert_allclose(np.array(rows), fresh, rtol=1e-11, atol=0)
    finally:
        os.unlink(ini)
