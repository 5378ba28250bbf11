"""CPU reference of the self-consistent exchange-only KLI step of include/dftatom_hip.h (dfta_scf_set_exchange): tests/_scf_ref.ScfRef
with its xc stage replaced by the exchange stage of tests/_exchange_ref.py on the step's own orbitals.  No GPU, no library.

The stages of the rule are separate functions, each in float64 with one IEEE operation per stated operation, so that a test can feed
each one the GPU's own input and ask for the GPU's bits:

    tail(v, D, r)                 v_raw beyond the last node with D > 0: (v_il r_il) / r_i
    mix(vx, v_raw, first, alpha)  vx = v_raw on the first step, alpha vx + (1 - alpha) v_raw later
    assemble(...)                 Vexc / va / vb / eexc from vx and the mixed densities
    ex_channel, ex_atom           E_x,sigma = 0.5 Sum n vbarHF (one accumulator), E_x = 2 E_x,0 or E_x,alpha + E_x,beta
    solve(M, vS, vHF, homo)       the device solve: the elimination order of the header in float64
    energies9(...)                the nine energies of dfta_energies from the step's arrays, eExcDif = 4 pi I[2] + E_x

and the Python statement of dftatom_amd/csrc/kli_plan.cpp (plan_channels, budget_rows, plan_chunks, capacities).
"""
import math

import numpy as np

import _exchange_ref as X
import _oracle as O
import _scf_ref as SR

LD = X.LD
FOURPI = SR.FOURPI

# exchange-only KLI total energies of the literature, Ha, four decimals (Krieger, Li, Iafrate 1992 and later tables); H and He exact / HF
LITERATURE = {"Li": -7.4324, "Be": -14.5723, "N": -54.4030, "Ne": -128.5448, "Ar": -526.8105}
E_H, E_HE_HF = -0.5, -2.8616800

# (Z, lsda) of the atoms tests/test_kli_scf_ref.py converges, by name
ATOMS = {"H": (1, True), "He": (2, False), "Li": (3, True), "Be": (4, False), "N": (7, True), "Ne": (10, False), "Ar": (18, False)}
GRID = (12, 2e-3, 25.0)                  # 4097 nodes: mg_levels, delta, Rmax

# MEASURED on the CPU reference at GRID, mix 0.5 (tests/test_kli_scf_ref.py holds each to [measured / 1.2, 1.2 x measured], or to an
# upper bound where the figure is round-off): the distance of converged H (LSDA) from -0.5 Ha in energy and eigenvalue, of He from the
# Hartree-Fock energy; "sens": the exchange stage in np.longdouble against float64 on the same (float64) orbitals of Ne after three
# steps -- max |v_raw_ld - v_raw_64| / max |v_raw| and |E_x_ld - E_x_64| / |E_x| -- the figure the GPU whole-step gates lean on;
# "tail_Ne": r vx at the last node of converged Ne.
MEASURED = {"H_E": 3.6e-08, "H_eps": 7.2e-08, "He_E": 2.4e-07, "tail_Ne": 7.8e-04, "sens": {"v_raw": 1.9e-15, "Ex": 3.8e-16}}


# ---- the stages, float64 ------------------------------------------------------------------------------------------------------------
def last_node(D):
    """the largest node with D > 0, or -1"""
    nz = np.nonzero(np.asarray(D) > 0)[0]
    return int(nz[-1]) if len(nz) else -1


def tail(v, D, r):
    """v with the Coulomb tail beyond the last node with D > 0 (one product, one quotient); nodes before it are untouched"""
    v = np.array(v, dtype=np.float64)
    il = last_node(D)
    if il >= 0 and il + 1 < len(v):
        v[il + 1:] = (v[il] * np.float64(r[il])) / np.asarray(r[il + 1:], dtype=np.float64)
    return v


def mix(vx, v_raw, first, alpha):
    if first:
        return np.array(v_raw, dtype=np.float64)
    a, b = np.float64(alpha), np.float64(1.) - np.float64(alpha)
    return a * np.asarray(vx, dtype=np.float64) + b * np.asarray(v_raw, dtype=np.float64)


def assemble(lsda, vxa, vxb=None, dA=None, dB=None, rho=None):
    """(Vexc, va, vb, eexc); LDA: va, vb None"""
    if not lsda:
        V = np.array(vxa, dtype=np.float64)
        return V, None, None, -V
    num = dA * vxa + dB * vxb
    V = np.zeros_like(num)
    ok = rho > 0
    V[ok] = num[ok] / rho[ok]
    return V, np.array(vxa), np.array(vxb), -V


def ex_channel(occ, vbarHF):
    acc = np.float64(0.)
    for n, v in zip(occ, vbarHF):
        acc = acc + np.float64(n) * np.float64(v)
    return np.float64(0.5) * acc


def ex_atom(lsda, exs):
    return exs[0] + exs[1] if lsda else np.float64(2.) * exs[0]


def solve(M, vS, vHF, homo):
    """the device solve (k_kli_solve): the header's elimination order, float64"""
    return X.solve_kli(np.asarray(M, dtype=np.float64), np.asarray(vS, dtype=np.float64), np.asarray(vHF, dtype=np.float64), homo,
                       dtype=np.float64)


def exchange_stage(U, l, occ, E, r, s, dtype=np.float64):
    """the stage on one channel: dict with v_raw (tail applied), vKLI (before the tail), D, vbarHF, c, homo, Ex -- in `dtype`"""
    U = np.asarray(U)
    if U.shape[0] == 0:
        N = len(r)
        return {"v_raw": np.zeros(N, dtype=dtype), "vKLI": np.zeros(N, dtype=dtype), "D": np.zeros(N, dtype=dtype),
                "vbarHF": np.zeros(0, dtype=dtype), "c": np.zeros(0, dtype=dtype), "homo": -1, "Ex": dtype(0)}
    homo = X.pick_homo(E, occ)
    p = X.potentials(U, l, occ, homo, np.asarray(r, dtype=dtype), np.asarray(s, dtype=dtype), dtype=dtype)
    v = np.array(p["vKLI"], dtype=dtype)
    il = last_node(p["D"])
    rr = np.asarray(r, dtype=dtype)
    if il >= 0 and il + 1 < len(v):
        v[il + 1:] = (v[il] * rr[il]) / rr[il + 1:]
    ex = dtype(0)
    for n, vb in zip(occ, p["vbar"][:, X.HF]):
        ex = ex + dtype(n) * vb
    return {"v_raw": v, "vKLI": p["vKLI"], "D": p["D"], "vbarHF": p["vbar"][:, X.HF], "c": p["c"], "homo": homo, "Ex": dtype(0.5) * ex}


def energies9(o, Z, lsda, pos, cnst, density, dA, dB, U, Vexc, eexc, potA, potB, Eel, Ex):
    """the nine energies of dfta_energies in k_tail's / k_energies' operation order (logarithmic grid), eExcDif = 4 pi I[2] + E_x"""
    N = len(pos)
    nuclear, exccor, eexcD, hartree, potentiale = (np.zeros(N) for _ in range(5))
    p, c, rho, Uu = pos[1:], cnst[1:], density[1:], U[1:]
    if not lsda:
        positiondensity = p * rho * c
        position2density = p * p * rho * c
        potentiale[1:] = position2density * potA[1:]
    else:
        positioncnst = p * c
        positiondensity = positioncnst * rho
        position2cnst = p * positioncnst
        position2density = position2cnst * rho
        potentiale[1:] = (position2cnst * dA[1:]) * potA[1:] + (position2cnst * dB[1:]) * potB[1:]
    nuclear[1:] = Z * positiondensity
    exccor[1:] = position2density * Vexc[1:]
    eexcD[1:] = position2density * eexc[1:]
    hartree[1:] = positiondensity * Uu
    s38 = lambda a: o.dfo_simpson38(1, O.dp(np.ascontiguousarray(a)), N)      # noqa: E731
    Enuclear = -FOURPI * s38(nuclear)
    Exc = FOURPI * s38(exccor)
    eExcDif = FOURPI * s38(eexcD) + Ex
    Exc += eExcDif
    Ehartree = -2 * math.pi * s38(hartree)
    Epotential = FOURPI * s38(potentiale)
    Ekinetic = Eel - Epotential
    Etotal = Eel + Ehartree + eExcDif
    return {"Etotal": Etotal, "Ekinetic": Ekinetic, "Ecoul": -Ehartree, "Enuclear": Enuclear, "Exc": Exc, "Eelectronic": Eel,
            "Ehartree": Ehartree, "eExcDif": eExcDif, "Epotential": Epotential}


def finished(Eold, Etotal, conv, last_time_converged):
    """the stop test of k_energies"""
    return abs((Eold - Etotal) / Etotal) < 1e-11 and bool(conv) and bool(last_time_converged)


class KliScfRef(SR.ScfRef):
    """ScfRef under DFTA_EXCHANGE_KLI: VWN start potential, then every step's exchange from its own orbitals.  dtype: the floating type of
    the exchange stage (the orbitals stay the oracle's float64)."""

    def __init__(self, Z, alpha, beta=None, mg_levels=GRID[0], mix=0.5, MaxR=GRID[2], delta=GRID[1], dtype=np.float64):
        super().__init__(Z, alpha, beta, functional=SR.VWN, mg_levels=mg_levels, mix=mix, MaxR=MaxR, delta=delta)
        self.dtype = dtype
        self.steps = 0
        self.orbs = [np.zeros((len(c), self.N)) for c in self.cfg]
        self.vx = [np.zeros(self.N), np.zeros(self.N)]
        self.v_raw = [np.zeros(self.N), np.zeros(self.N)]
        self.Ex, self.stage = 0.0, [None, None]
        self.s = self.cnst_xc                                                      # dr/di at every node

    def channel_occ(self, spin):
        return [f if self.lsda else 0.5 * f for _, _, f in self.cfg[spin]]

    def solve_channel(self, pot, spin):
        """level search on pot: eigenvalues, orbitals (kept), Sum f Psi^2, Sum f E, converged"""
        levels = self.cfg[spin]
        found = [self.eigenvalue(pot, n, l) for n, l, _ in levels]
        E = np.array([e for e, _ in found])
        acc, eel = np.zeros(self.N), 0.0
        U = np.zeros((len(levels), self.N))
        for k, ((n, l, f), e) in enumerate(zip(levels, E)):
            U[k] = self.orbital(pot, l, e)
            acc[:-1] += (f * U[k][:-1]) * U[k][:-1]
            eel += f * e
        self.orbs[spin] = U
        return E, acc, eel, all(c for _, c in found)

    def exchange(self, spin, dtype=None):
        """the exchange stage of channel `spin` on the orbitals of the last level search"""
        l = [x for _, x, _ in self.cfg[spin]]
        return exchange_stage(self.orbs[spin], l, self.channel_occ(spin), self.E[spin], self.pos, self.s, dtype=dtype or self.dtype)

    def step(self):
        Eel = 0.0
        nspin = 2 if self.lsda else 1
        if not self.lsda:
            self.E[0], acc, e, conv = self.solve_channel(self.potA, 0)
            Eel += e
            self.density = self.mix(self.density, acc)
        else:
            self.E[0], acc, e, c1 = self.solve_channel(self.potA, 0)
            Eel += e
            self.dA = self.mix(self.dA, acc)
            self.E[1], acc, e2, c2 = self.solve_channel(self.potB, 1)
            for (_, _, f), E in zip(self.cfg[1], self.E[1]):
                Eel += f * E
            self.dB = self.mix(self.dB, acc)
            conv = c1 and c2
            self.density = self.density.copy()
            self.density[1:] = self.dA[1:] + self.dB[1:]
        self.steps += 1
        exs = []
        for sp in range(nspin):
            st = self.exchange(sp)
            self.stage[sp] = st
            self.v_raw[sp] = np.asarray(st["v_raw"], dtype=np.float64)
            self.vx[sp] = mix(self.vx[sp], self.v_raw[sp], self.steps == 1, self.alpha_mix)
            exs.append(np.float64(st["Ex"]))
        self.Ex = float(ex_atom(self.lsda, exs))
        self.U = self.poisson(self.density, self.Ne)
        self.Vexc, va, vb, self.eexc = assemble(self.lsda, self.vx[0], self.vx[1], self.dA, self.dB, self.density)
        if self.lsda:
            self.va, self.vb = va, vb
        self.potA, self.potB = self.potentials(self.U, self.Vexc, self.va, self.vb)
        en = energies9(self.o, self.Z, self.lsda, self.pos, self.cnst, self.density, self.dA, self.dB, self.U, self.Vexc, self.eexc,
                       self.potA, self.potB, Eel, self.Ex)
        self.en = en
        if finished(self.Eold, en["Etotal"], conv, self.lastTimeConverged):
            self.finished = 1
        else:
            self.Eold, self.lastTimeConverged = en["Etotal"], int(bool(conv))
        return [en[k] for k in ("Etotal", "Ekinetic", "Ecoul", "Enuclear", "Exc")]

    def run(self, cap=60):
        """steps until finished, at most cap; the number of steps taken"""
        while not self.finished and self.steps < cap:
            self.step()
        return self.steps


def aufbau_config(Z, lsda):
    """(alpha, beta) level lists of the Aufbau configuration of Z as ScfRef takes them, from the library's host-only tables"""
    import dftatom_amd as D
    return SR.config_levels(D.ion_config(Z, 0, lsda), lsda)


def make(name, dtype=np.float64, **kw):
    Z, lsda = ATOMS[name]
    a, b = aufbau_config(Z, lsda)
    return KliScfRef(Z, a, b, dtype=dtype, **kw)


# ---- the Python statement of dftatom_amd/csrc/kli_plan.cpp -----------------------------------------------------------------------------
def plan_channels(norb, l, occ, atom=None):
    """(channels, jobs): channels as tuples u0, norb, job0, njobs, first0, tab0, ntab, red0, nred, atom; jobs (x, y, k) on the batch's rows"""
    chans, jobs = [], []
    u0 = first0 = tab0 = red0 = 0
    for c, n in enumerate(norb):
        lc = list(l[u0:u0 + n])
        yj = X.y_jobs(lc) if n else []
        ntab = sum(len(e) for e in X.x_entries(lc)) if n else 0
        nred = 2 * n + n * (n + 1) // 2 if n else 0
        chans.append((u0, n, len(jobs), len(yj), first0, tab0, ntab, red0, nred, -1 if atom is None else atom[c]))
        jobs += [(u0 + x, u0 + y, k) for x, y, k in yj]
        u0, first0, tab0, red0 = u0 + n, first0 + (n + 1 if n else 0), tab0 + ntab, red0 + nred
    return chans, jobs


def budget_rows(mb, N):
    return int(math.floor(mb * 1048576. / (8. * N))) if mb > 0 else 0


def plan_chunks(njobs, live, max_rows):
    """pairs (c0, c1) over channels with njobs[c] y jobs each"""
    out, c0, rows = [], -1, 0

    def close(c1):
        nonlocal c0, rows
        if c0 >= 0 and rows > 0:
            out.append((c0, c1))
        c0, rows = -1, 0
    for c, n in enumerate(njobs):
        if live is not None and not live[c]:
            close(c)
            continue
        if c0 >= 0 and rows > 0 and rows + n > max_rows:
            close(c)
        if c0 < 0:
            c0 = c
        rows += n
    close(len(njobs))
    return out


def capacities(njobs, norb, max_rows):
    y = min(sum(njobs), max(max(njobs, default=0), max_rows))
    return y, min(sum(norb), y), len(njobs)
