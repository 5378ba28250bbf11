"""CPU reference of the SCF step with Anderson density mixing (include/dftatom_hip.h, DFTA_MIX_ANDERSON): tests/_scf_ref.ScfRef
with the mixing stage replaced, in float64 numpy on ScfRef's own stage methods.

Per step k = 1, 2, ... of the atom: x the input density (LSDA: dA and dB joined into one vector), g = Sum f Psi^2 / (4 pi r^2) the
output density, f = g - x, node 0 excluded, lin = ScfRef.mix (the linear mix, ScfRef's bits).  The (x, f) pairs of the newest m
previous steps are kept, recorded from step 1 on.  k <= warmup or no history: x+ = lin.  Otherwise, over the stored pairs oldest to
newest, dX_j = x - x_j, dF_j = f - f_j, <u, v> = Sum w u v with w = 4 pi r^2 dr/di over both channels,
    (A + 1e-14 trace(A) I) gamma = b,   A_jk = <dF_j, dF_k>,   b_j = <dF_j, f>           (Cholesky, column by column)
    cand = lin - Sum_j gamma_j (dX_j + (1 - alpha) dF_j);   x+ = cand where cand >= 0, lin elsewhere.
A pivot <= 0 or a non-finite gamma: x+ = lin, and the history is cleared (this step's pair is not kept either).
With mixing off every step is ScfRef.step itself.
"""
import math

import numpy as np

import _scf_ref as SR
from _scf_ref import FOURPI, ScfRef


def cholesky_solve(A, b):
    """gamma of A gamma = b, or None: a pivot <= 0 or a non-finite gamma"""
    h = len(b)
    L = np.zeros((h, h))
    for j in range(h):
        p = A[j, j]
        for q in range(j):
            p -= L[j, q] * L[j, q]
        if not p > 0.0:
            return None
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, h):
            s = A[i, j]
            for q in range(j):
                s -= L[i, q] * L[j, q]
            L[i, j] = s / L[j, j]
    y = np.zeros(h)
    for i in range(h):
        s = b[i]
        for q in range(i):
            s -= L[i, q] * y[q]
        y[i] = s / L[i, i]
    for i in range(h - 1, -1, -1):
        s = y[i]
        for q in range(i + 1, h):
            s -= L[q, i] * y[q]
        y[i] = s / L[i, i]
    return y if np.all(np.isfinite(y)) else None


class AndersonRef(ScfRef):
    def __init__(self, *args, mixing=True, m=4, warmup=3, **kw):
        super().__init__(*args, **kw)
        self.mixing, self.m, self.warmup = bool(mixing), int(m), int(warmup)
        self.k = 0
        self.hist = []                       # (x, f) of the previous steps, oldest first, nodes 1 .. N-1 of every channel joined
        self.accelerated = 0                 # steps that took the accelerated mix
        self.cleared = 0                     # failed solves
        nch = 2 if self.lsda else 1
        self.w = np.tile(FOURPI * self.pos[1:] * self.pos[1:] * self.cnst[1:], nch)

    def anderson_mix(self, xs, accs):
        """the new densities of the channels from their input densities xs and the level solver's Sum f Psi^2 accs"""
        lins = [ScfRef.mix(self, x, acc) for x, acc in zip(xs, accs)]
        p = self.pos[1:]
        X = np.concatenate([x[1:] for x in xs])
        G = np.concatenate([acc[1:] / (FOURPI * p * p) for acc in accs])
        F = G - X
        LIN = np.concatenate([lin[1:] for lin in lins])
        self.k += 1
        new, keep = LIN, True
        if self.k > self.warmup and self.hist:
            beta = 1. - self.alpha_mix
            dX = [X - xj for xj, _ in self.hist]
            dF = [F - fj for _, fj in self.hist]
            h = len(dF)
            A = np.array([[np.sum(self.w * dF[j] * dF[k]) for k in range(h)] for j in range(h)])
            b = np.array([np.sum(self.w * dF[j] * F) for j in range(h)])
            gamma = cholesky_solve(A + 1e-14 * np.trace(A) * np.eye(h), b)
            if gamma is None:
                self.hist, keep = [], False
                self.cleared += 1
            else:
                s = np.zeros_like(LIN)
                for j in range(h):
                    s += gamma[j] * (dX[j] + beta * dF[j])
                cand = LIN - s
                new = np.where(cand >= 0., cand, LIN)
                self.accelerated += 1
        if keep:
            self.hist = (self.hist + [(X, F)])[-self.m:]
        outs, n = [], self.N - 1
        for c, x in enumerate(xs):
            o = x.copy()
            o[1:] = new[c * n:(c + 1) * n]
            outs.append(o)
        return outs

    def step(self):
        if not self.mixing:
            return ScfRef.step(self)
        Eel = 0.0
        if not self.lsda:
            self.E[0], acc, e, conv = self.solve_levels(self.potA, self.cfg[0])
            Eel += e
            self.density, = self.anderson_mix([self.density], [acc])
        else:
            self.E[0], accA, e, c1 = self.solve_levels(self.potA, self.cfg[0])
            Eel += e
            self.E[1], accB, _, c2 = self.solve_levels(self.potB, self.cfg[1])
            for (_, _, f), E in zip(self.cfg[1], self.E[1]):                       # one running sum over both channels, as ScfRef's
                Eel += f * E
            self.dA, self.dB = self.anderson_mix([self.dA, self.dB], [accA, accB])
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


def run_to_finish(ref, cap=100):
    """steps until the reference's stop test: (steps, energies of the last step)"""
    n, en = 0, None
    while not ref.finished:
        assert n < cap, n
        en = ref.step()
        n += 1
    return n, en


__all__ = ["AndersonRef", "cholesky_solve", "run_to_finish", "SR"]
