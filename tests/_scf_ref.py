"""CPU reference of one SCF step for any functional, any (fractional) occupations and any electron count: tests/_ion_ref.IonScf
generalised, from the oracle's own primitives (tests/_oracle.py) and tests/_gga_ref.py.

* occupations are doubles: every level is solved on its own by dfo_loop_over_levels (one level, the clamped un-chained brackets
  of the GPU's default path, occupation 0, a scratch density) for its eigenvalue, dfo_match + dfo_normalize_nonuniform give Psi,
  and acc += (f Psi) Psi for i < N-1 in level order is done here -- the operation order of dfo_loop_over_levels and of
  k_accumulate_density; Eel += f E;
* the electron count is a double: dfo_solve_poisson_nonuniform restated on the oracle's multigrid (poisson());
* the functional is a plug: VWN through the oracle's dfo_vwn_*, PW92 and PBE through _gga_ref.radial.

With VWN and integer occupations every stage keeps the oracle's operation order, so a step returns the bits of IonScf, hence of
dfo_scf_step (tests/test_scf_ref.py).  The stages (solve_levels, mix, poisson, xc, potentials, energies) are separate methods so
that a test can feed each one the GPU's own input to that stage.  Logarithmic grid only.
"""
import ctypes as C
import math

import numpy as np

import _gga_ref as R
import _oracle as O

FOURPI = 4. * math.pi
VWN, PW92, PBE = 0, R.PW92, R.PBE            # DFTA_XC_VWN, DFTA_XC_PW92, DFTA_XC_PBE


def config_levels(cfg, lsda):
    """a configuration of dftatom_amd.parse_config / ion_config as (alpha, beta) lists of (n, l, f); LDA: beta None"""
    to = lambda ls: [(int(n), int(l), float(f)) for n, l, f in ls]                 # noqa: E731
    return to(cfg["alpha"]), (to(cfg["beta"]) if lsda else None)


class ScfRef:
    """alpha / beta: lists of (n, l, f), n as the oracle counts it (principal quantum number - 1), f a double; LDA: beta None"""

    def __init__(self, Z, alpha, beta=None, functional=VWN, mg_levels=14, mix=0.5, MaxR=25.0, delta=5e-4):
        o = O.oracle()
        self.o, self.Z, self.lsda, self.alpha_mix, self.MaxR, self.delta = o, int(Z), beta is not None, mix, MaxR, delta
        self.functional, self.mg_levels = functional, mg_levels
        self.g = O.make_grid(mg_levels, delta, MaxR)
        N = self.N = self.g.N
        self.ps = o.dfo_poisson_create(mg_levels, delta)
        self.cfg = [list(alpha), list(beta or [])]
        self.E = [np.zeros(len(c)) for c in self.cfg]
        na = math.fsum(f for _, _, f in self.cfg[0])
        nb = math.fsum(f for _, _, f in self.cfg[1])
        self.Ne = na + nb
        assert 0 < self.Ne <= self.Z
        self.pos = np.array([0.0] + [self.g.Rp * (math.exp(i * delta) - 1.) for i in range(1, N)])
        self.cnst = np.array([0.0] + [self.g.Rp * delta * math.exp(delta * i) for i in range(1, N)])
        self.cnst_xc = self.cnst.copy()                                            # the stencils divide by dr/di at node 0 as well
        self.cnst_xc[0] = self.g.Rp * delta
        z = np.zeros
        self.density, self.dA, self.dB, self.U = z(N), z(N), z(N), z(N)
        volume = FOURPI / 3. * MaxR * MaxR * MaxR
        if not self.lsda:
            self.density[1:] = self.Ne / volume
        else:
            self.dA[1:], self.dB[1:] = na / volume, nb / volume
            self.density[1:] = na / volume + nb / volume
        self.U = self.poisson(self.density, self.Ne)
        self.Vexc, self.va, self.vb, self.eexc = self.xc(self.density, self.dA, self.dB)
        self.potA, self.potB = self.potentials(self.U, self.Vexc, self.va, self.vb)
        self.Eold, self.lastTimeConverged, self.finished = 0.0, 0, 0

    def close(self):
        if self.ps:
            self.o.dfo_poisson_destroy(self.ps)
            self.ps = None

    def levels(self, spin=0):
        return self.E[spin].copy()

    # ---- the stages ----------------------------------------------------------------------------------------------------------
    def eigenvalue(self, pot, n, l):
        """one level on potential pot: (E, converged)"""
        lev = (O.Level * 1)()
        lev[0].n, lev[0].l, lev[0].occ = n, l, 0
        bottom = C.c_double(-float(self.Z) * self.Z - 1.)
        scratch, eel = np.zeros(self.N), C.c_double(0.0)
        conv = self.o.dfo_loop_over_levels(C.byref(self.g), O.dp(pot), lev, 1, O.dp(scratch), C.byref(eel), C.byref(bottom), 3, None)
        return lev[0].E, conv

    def orbital(self, pot, l, E):
        """normalised Psi of the oracle at energy E"""
        psi = np.zeros(self.N)
        self.o.dfo_match(C.byref(self.g), O.dp(pot), l, float(E), O.dp(psi), None)
        self.o.dfo_normalize_nonuniform(C.byref(self.g), O.dp(psi))
        return psi

    def accumulate(self, pot, levels, energies):
        """Sum f Psi^2 over the levels at the given energies (nodes 0 .. N-2, level order) and Sum f E, added in level order"""
        acc, eel = np.zeros(self.N), 0.0
        for (n, l, f), E in zip(levels, energies):
            psi = self.orbital(pot, l, E)
            acc[:-1] += (f * psi[:-1]) * psi[:-1]
            eel += f * E
        return acc, eel

    def solve_levels(self, pot, levels):
        """(eigenvalues, Sum f Psi^2, Sum f E, all converged)"""
        found = [self.eigenvalue(pot, n, l) for n, l, _ in levels]
        E = np.array([e for e, _ in found])
        acc, eel = self.accumulate(pot, levels, E)
        return E, acc, eel, all(c for _, c in found)

    def mix(self, density, acc):
        """alpha rho + (1 - alpha) acc / (4 pi r^2), nodes 1 .. N-1 (dfo_calculate_density); node 0 keeps its value"""
        out = density.copy()
        p = self.pos[1:]
        out[1:] = self.alpha_mix * density[1:] + (1. - self.alpha_mix) * (acc[1:] / (FOURPI * p * p))
        return out

    def poisson(self, density, Ne):
        """dfo_solve_poisson_nonuniform with a double at the boundary U(Rmax)"""
        p = self.ps.contents
        size, d = p.n[0], p.deltaGrid
        src = np.ctypeslib.as_array(p.Src[0], (size,))
        Rp = self.MaxR / (math.exp((size - 1) * d) - 1.)
        src[:] = [Rp * (math.exp(i * d) - 1.) for i in range(size)]
        delta2grid = d * d
        Rp2delta2 = Rp * Rp * delta2grid
        twodelta = 2. * d
        c = FOURPI * Rp2delta2
        lim = size - 1
        e = np.array([math.exp(i * twodelta) for i in range(1, lim)])
        src[1:lim] *= c * e * density[1:lim]
        p.lowB, p.highB = 0.0, float(Ne)
        self.o.dfo_full_cycle(self.ps, 1E-3, 1E-14)
        return np.ctypeslib.as_array(p.Phi[0], (size,)).copy()

    def xc(self, density, dA=None, dB=None, dtype=None):
        """(Vexc, va, vb, eexc); LDA: va, vb are zeros.  dtype: evaluate PW92 / PBE in that floating type (np.longdouble)"""
        o, N = self.o, self.N
        Vexc, va, vb, eexc = (np.zeros(N) for _ in range(4))
        if self.functional == VWN:
            if not self.lsda:
                o.dfo_vwn_vexc(O.dp(density), O.dp(Vexc), N)
                o.dfo_vwn_eexcdif(O.dp(density), O.dp(eexc), N)
            else:
                o.dfo_vwn_vexc_lsda(O.dp(dA), O.dp(dB), O.dp(Vexc), O.dp(va), O.dp(vb), N)
                o.dfo_vwn_eexcdif_lsda(O.dp(dA), O.dp(dB), O.dp(eexc), N)
            return Vexc, va, vb, eexc
        cast = (lambda x: x) if dtype is None else (lambda x: x.astype(dtype))     # noqa: E731
        if not self.lsda:
            Vexc, eexc = R.radial(self.functional, self.pos, self.cnst_xc, cast(density))
            return Vexc, np.zeros_like(Vexc), np.zeros_like(Vexc), eexc
        return tuple(R.radial(self.functional, self.pos, self.cnst_xc, cast(dA), cast(dB)))

    def potentials(self, U, Vexc, va, vb):
        potA, potB = np.zeros(self.N), np.zeros(self.N)
        u = (-self.Z + U[1:]) / self.pos[1:]
        if not self.lsda:
            potA[1:] = u + Vexc[1:]
        else:
            potA[1:] = u + va[1:]
            potB[1:] = u + vb[1:]
        return potA, potB

    def energies(self, density, dA, dB, U, Vexc, eexc, potA, potB, Eel):
        """(Etotal, Ekinetic, Ecoul, Enuclear, Exc) in dfo_scf_step's operation order"""
        N, Zi = self.N, self.Z
        nuclear, exccor, eexcD, hartree, potentiale = (np.zeros(N) for _ in range(5))
        p, c, rho, U = self.pos[1:], self.cnst[1:], density[1:], U[1:]
        if not self.lsda:
            positiondensity = p * rho * c
            position2density = p * p * rho * c
            potentiale[1:] = position2density * potA[1:]
        else:
            positioncnst = p * c
            positiondensity = positioncnst * rho
            position2cnst = p * positioncnst
            position2density = position2cnst * rho
            potentiale[1:] = (position2cnst * dA[1:]) * potA[1:] + (position2cnst * dB[1:]) * potB[1:]
        nuclear[1:] = Zi * positiondensity
        exccor[1:] = position2density * Vexc[1:]
        eexcD[1:] = position2density * eexc[1:]
        hartree[1:] = positiondensity * U
        s38 = lambda a: self.o.dfo_simpson38(1, O.dp(np.ascontiguousarray(a)), N)      # noqa: E731
        Enuclear = -FOURPI * s38(nuclear)
        Exc = FOURPI * s38(exccor)
        eExcDif = FOURPI * s38(eexcD)
        Exc += eExcDif
        Ehartree = -2 * math.pi * s38(hartree)
        Epotential = FOURPI * s38(potentiale)
        Ekinetic = Eel - Epotential
        Etotal = Eel + Ehartree + eExcDif
        return [Etotal, Ekinetic, -Ehartree, Enuclear, Exc]

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def step(self):
        """one SCF step from the object's own state; returns the five energies"""
        Eel = 0.0
        if not self.lsda:
            self.E[0], acc, e, conv = self.solve_levels(self.potA, self.cfg[0])
            Eel += e
            self.density = self.mix(self.density, acc)
        else:
            self.E[0], acc, e, c1 = self.solve_levels(self.potA, self.cfg[0])
            Eel += e
            self.dA = self.mix(self.dA, acc)
            self.E[1], acc, e2, c2 = self.solve_levels(self.potB, self.cfg[1])
            for (_, _, f), E in zip(self.cfg[1], self.E[1]):                       # one running sum over both channels, as the oracle's
                Eel += f * E
            self.dB = self.mix(self.dB, acc)
            conv = c1 and c2
            self.density = self.density.copy()
            self.density[1:] = self.dA[1:] + self.dB[1:]
        self.U = self.poisson(self.density, self.Ne)
        self.Vexc, self.va, self.vb, self.eexc = self.xc(self.density, self.dA, self.dB)
        self.potA, self.potB = self.potentials(self.U, self.Vexc, self.va, self.vb)
        en = self.energies(self.density, self.dA, self.dB, self.U, self.Vexc, self.eexc, self.potA, self.potB, Eel)
        Etotal = en[0]
        if abs((self.Eold - Etotal) / Etotal) < 1e-11 and conv and self.lastTimeConverged:
            self.finished = 1
        else:
            self.Eold, self.lastTimeConverged = Etotal, int(bool(conv))
        return en
