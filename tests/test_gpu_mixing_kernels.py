"""GPU suite (-m gpu): the three launches of the Anderson density mixing -- k_anderson_gram, k_anderson_solve, k_anderson_update
(dftatom_amd/csrc/mixing.hip) -- stage by stage through dfta_mixer (dftatom_amd.Mixer), against tests/_mix_ref.py evaluated in
EXTENDED precision (np.longdouble; anchored to AndersonRef in tests/test_mix_ref.py).  After every step each stage is checked from
the DEVICE's own input to that stage (the ring read back before the step, the device's slab, the device's gamma): nothing compounds.
eps = 2^-52 throughout.

a. g     acc comes back as acc / fpr2 bit for bit, node 0 and the rows of a frozen atom untouched.
b. slab  every used dot d < H (H + 1) / 2 + H of every chunk against the extended sum over that chunk's nodes (1 <= i < N, both
         channels), to c eps T_chunk, T the sum of |term|.  c is the number of roundings on one term's way into the chunk's sum in the
         kernel's documented order: w = fpr2 (cnst hstep) 2, the products w dF_j and (w dF_j) dF_k 2, the thread's accumulation over
         channel, then node, 4 nodes per thread and channel: 4 (LDA) / 8 (LSDA), the six xor-shuffle levels 6, the tree
         (w0 + w1) + (w2 + w3) 2:  c = 16 (LDA), 20 (LSDA).  f and dF_j are float64 differences of the stage's inputs and shared bit
         for bit.  Entries d >= nd are not compared.
c. solve A and b are the slab summed chunk 0, 1, ... on the host in float64.  With A_r = A + 1e-14 trace(A) I (float64, as the kernel
         forms it) the residual, evaluated in extended precision, obeys ||b - A_r gamma||_2 <= H (3H + 1) eps ||A_r||_2 ||gamma||_2
         (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4 with || |R^T| |R| || <= H ||A||): independent of
         conditioning.  The shift itself, which that bound cannot see: at H = 1, gamma = b / (a (1 + 1e-14)) to 4 eps relative (one
         add, one sqrt, two divisions; without the shift it is 45 eps away).  The eight state ints equal _mix_ref.automaton's; gamma
         is eight zeros on a linear step.
d. duplicate pair: two bitwise equal pairs, A exactly singular before the shift: the solve succeeds, the step passes c and e, and
         gamma_0 + gamma_1 -- which the system determines although it does not determine gamma_0 - gamma_1 -- is compared with its
         exact value 2 b_0 / (2 A_00 + lambda) (the sum of the two equations (A_00 + lambda) gamma_0 + A_00 gamma_1 = b_0 and its
         mirror image), to eight times the distance of _anderson_ref.cholesky_solve, run in float64 on the same dots, from it.
e. update every node of every channel against the extended candidate built from the device's gamma, to c' eps T with
         T = |alpha x| + |(1 - alpha) g| + Sum_j |gamma_j| (|dX_j| + (1 - alpha) |dF_j|).  c' counts mixed()'s roundings on the
         longest path of a term: (1 - alpha) dF_j 1, dX_j + that 1, gamma_j times it 1, the sum over j: H, lin - s 1:  c' = H + 4
         (lin's own path, alpha x, the add, the subtraction, is 3; dX_j and dF_j are float64 differences shared bit for bit; the
         library is built without FMA contraction).  Clamp: cand_ext < -tol: the output is lin, bit for bit; cand_ext > tol: the
         candidate; inside the band: one of the two.  The band may hold 0.1 % of a case's nodes (the generator gives none on the
         model), and every case must hold clearly negative candidates.  LSDA: density = dA + dB bit for bit.  lin is the output of a
         DFTA_MIX_LINEAR mixer -- the k_mix launch itself -- on the same inputs; warm-up and failed-solve steps equal it bit for bit.
f. ring  after a step slot `head` holds (x, g - x) bit for bit; every other slot, and every slot of a frozen atom, keeps its bits.

A non-finite acc node is plain data: its chunk's dots are non-finite, the solve fails, the step is the linear one (finite everywhere
else), the history is cleared.

Every test prints the largest ratio to each bound that it observed.  NOT YET RUN ON AN MI355X: no device figures are recorded
here, and none of the assertions below has been seen to pass or fail on the kernels.  With the float64 model of _mix_ref.py standing in for the device
(NumPy's pairwise sums, no kernel) the same assertions give: slab <= 0.13, solve residual <= 0.33, H = 1 shift <= 0.28, update <= 0.20
of the respective bound, 0 nodes in the clamp's band, 288 .. 21 135 clearly negative candidates per case.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _anderson_ref as AR               # noqa: E402
import _mix_ref as M                     # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD = M.LD
EPS = M.EPS
ALPHA = M.ALPHA


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


_grids = {}


@pytest.fixture(scope="module")
def grids(ctx):
    """(grid, r, fpr2, w) by (N, uniform): r from the library, the weights by the grid's own formulas"""
    def get(N, uniform=False):
        if (N, uniform) not in _grids:
            L, delta = M.LOG_GRIDS[N]
            g = D.Grid(ctx, L, None if uniform else delta, M.RMAX)
            assert g.N == N
            r = g.r()
            tr, cnst, hstep = M.uniform_tables(N, M.RMAX) if uniform else M.log_tables(N, delta, M.RMAX, Rp=g.Rp)
            assert np.array_equal(bits(r), bits(tr))
            _grids[(N, uniform)] = (g, r) + M.weights(r, cnst, hstep)
        return _grids[(N, uniform)]
    yield get
    for G in _grids.values():
        G[0].close()
    _grids.clear()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same(a, b):
    """bit for bit; a NaN matches a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


class Worst:
    """the largest observed ratio to each bound, and the clamp's counts"""

    def __init__(self):
        self.slab = self.solve = self.shift = self.update = 0.0
        self.neg = self.band = self.nodes = self.accelerated = self.failed = 0

    def line(self, label):
        return ("%-34s slab %.3f  solve residual %.3f  H = 1 shift %.3f  update %.3f  clamp: %d clearly negative, %d in the band, of %d "
                "(%.4f %%); %d accelerated steps, %d failed solves"
                % (label, self.slab, self.solve, self.shift, self.update, self.neg, self.band, self.nodes,
                   100.0 * self.band / max(self.nodes, 1), self.accelerated, self.failed))


def assemble(inputs, natoms, lsda, k, N):
    """the batch's arrays of step k: acc [atom][channel][N], density, dA, dB [atom][N], fin; node 0 carries markers"""
    nch = 2 if lsda else 1
    ACC, X, fin = np.zeros((natoms, nch, N)), np.zeros((natoms, nch, N)), np.zeros(natoms, np.int32)
    for a in range(natoms):
        x, acc, fin[a] = inputs(a, k)
        X[a], ACC[a] = x, acc
    ACC[:, :, 0] = 5.0
    X[:, :, 0] = (3.0, 4.0)[:nch]
    dens = X.sum(axis=1) if lsda else X[:, 0].copy()
    return ACC, X, dens, fin


def check_step(G, lsda, m, warmup, x, acc, fin, before, after, got, lin, worst, tag):
    """one atom, one step.  before / after: Mixer.get; got / lin: (g, density, dA, dB) rows of the Anderson / the linear mixer.
    Returns whether the solve failed."""
    _, r, fpr2, w = G
    nch, N = x.shape
    beta = 1. - ALPHA
    dens_in = x.sum(axis=0) if lsda else x[0]
    if fin:                                                          # frozen: nothing moves
        assert same(got[0], acc) and same(got[1], dens_in), tag
        if lsda:
            assert same(got[2], x[0]) and same(got[3], x[1]), tag
        for key in ("state", "gamma", "slab", "ring"):
            assert same(after[key], before[key]) if key != "state" else np.array_equal(after[key], before[key]), (tag, key)
        return False
    # a. g
    g, f = M.residual(x, acc, fpr2)
    assert g[0, 0] == 5.0 and same(got[0], g), (tag, "g", int(np.sum(bits(got[0]) != bits(g))))
    assert same(lin[0], g), (tag, "the linear mixer's g")
    # b. slab
    head, length, steps = (int(v) for v in before["state"][:3])
    H = 0 if steps + 1 <= warmup else length
    slots = M.history_slots(head, length, m, H)
    xh, fh = [before["ring"][:, s, 0] for s in slots], [before["ring"][:, s, 1] for s in slots]
    nd = M.n_dots(H)
    c_slab = 4 + 4 * nch + 6 + 2
    for c, (lo, hi) in enumerate(M.chunks_of(N) if H else []):
        val, T = M.gram_shares(w, f, fh, lo, hi)
        dev = after["slab"][c, :nd]
        for d in range(nd):
            if not np.isfinite(T[d]):
                assert not np.isfinite(dev[d]), (tag, "slab", c, d)
                continue
            err, tol = abs(LD(dev[d]) - val[d]), c_slab * EPS * T[d]
            assert err <= tol, (tag, "slab", c, d, float(err), float(tol))
            if tol > 0:
                worst.slab = max(worst.slab, float(err / tol))
    # c. solve
    dots = np.zeros(nd)
    with np.errstate(all="ignore"):
        for c in range(after["slab"].shape[0] if H else 0):
            dots = dots + after["slab"][c, :nd]
    A, b = M.unpack(dots, H)
    ok = H > 0 and M.solve(A, b) is not None
    st_after, this = M.automaton((head, length, steps), m, warmup, ok)
    assert after["state"].tolist() == M.state_ints(st_after, this), (tag, after["state"].tolist(), M.state_ints(st_after, this))
    gamma = after["gamma"]
    if not ok:
        assert np.all(bits(gamma) == 0), (tag, gamma)
    else:
        assert np.all(np.isfinite(gamma[:H])) and np.all(bits(gamma[H:]) == 0), (tag, gamma)
        Ar, lam = M.regularised(A)
        gl = gamma[:H].astype(LD)
        res = b.astype(LD) - np.array([np.sum(Ar[j].astype(LD) * gl) for j in range(H)], dtype=LD)
        bound = H * (3 * H + 1) * EPS * np.linalg.norm(Ar, 2) * float(np.sqrt(np.sum(gl * gl)))
        ratio = float(np.sqrt(np.sum(res * res))) / bound
        assert ratio <= 1.0, (tag, "solve residual", ratio)
        worst.solve = max(worst.solve, ratio)
        if H == 1:
            exact = LD(b[0]) / (LD(A[0, 0]) * (LD(1) + LD(M.SHIFT)))
            ratio = float(abs(LD(gamma[0]) - exact) / (4 * EPS * abs(exact)))
            assert ratio <= 1.0, (tag, "shift", ratio)
            worst.shift = max(worst.shift, ratio)
    # e. update
    out = np.stack([got[2], got[3]]) if lsda else got[1][None]
    lout = np.stack([lin[2], lin[3]]) if lsda else lin[1][None]
    assert same(out[:, 0], x[:, 0]) and got[1][0] == dens_in[0], (tag, "node 0")
    if lsda:
        assert same(got[1][1:], got[2][1:] + got[3][1:]), (tag, "density = dA + dB")
    if not ok:
        assert same(out, lout) and same(got[1], lin[1]), (tag, "a linear step")
        bad = ~np.isfinite(acc)
        assert np.all(np.isfinite(out[~bad])), tag
        worst.failed += int(H > 0)
    else:
        _, cand, T = M.candidate(ALPHA, beta, x, g, xh, fh, gamma[:H])
        tol = (H + 4) * EPS * T
        cand, tol, o, lo_ = cand[:, 1:], tol[:, 1:], out[:, 1:], lout[:, 1:]
        assert np.all(np.isfinite(o)), tag
        is_lin = bits(o) == bits(lo_)
        err = np.abs(o.astype(LD) - cand)
        is_cand = err <= tol
        neg, pos = cand < -tol, cand > tol
        assert np.all(is_lin[neg]), (tag, "clamp: negative candidates kept", int(np.sum(~is_lin[neg])))
        assert np.all(is_cand[pos]), (tag, "update", float(np.max(err[pos] / tol[pos])), int(np.sum(~is_cand[pos])))
        assert np.all((is_lin | is_cand)[~neg & ~pos]), (tag, "clamp band")
        if pos.any():
            worst.update = max(worst.update, float(np.max(err[pos] / tol[pos])))
        worst.neg += int(neg.sum())
        worst.band += int((~neg & ~pos).sum())
        worst.nodes += cand.size
        worst.accelerated += 1
    # f. ring
    want = before["ring"].copy()
    want[:, this[0], 0, 1:] = x[:, 1:]
    want[:, this[0], 1, 1:] = f[:, 1:]
    assert same(after["ring"], want), (tag, "ring")
    return H > 0 and not ok


def run_case(ctx, G, lsda, natoms, m, warmup, steps, inputs, label, checked=True):
    """drive an Anderson and a linear mixer over the case; checked: every stage of every atom after every step.  Returns (the largest
    ratios, per atom the steps of its failed solves, per step and atom a record of everything the device produced)."""
    grid, N = G[0], G[0].N
    mix = D.Mixer(ctx, grid, lsda, natoms, D.MIX_ANDERSON, m, warmup)
    linear = D.Mixer(ctx, grid, lsda, natoms, D.MIX_LINEAR)
    worst, failed, records = Worst(), {a: [] for a in range(natoms)}, []
    written = [set() for _ in range(natoms)]
    try:
        before = [mix.get(a) for a in range(natoms)]
        for k in range(1, steps + 1):
            ACC, X, dens, fin = assemble(inputs, natoms, lsda, k, N)
            dA, dB = (X[:, 0], X[:, 1]) if lsda else (None, None)
            got = mix.step(ALPHA, ACC, dens, dA, dB, fin)
            lin = linear.step(ALPHA, ACC, dens, dA, dB, fin)
            after = [mix.get(a) for a in range(natoms)]
            rec = []
            for a in range(natoms):
                row = lambda t: [None if v is None else v[a] for v in t]                       # noqa: E731
                if checked and check_step(G, lsda, m, warmup, X[a], ACC[a], int(fin[a]), before[a], after[a], row(got), row(lin), worst,
                                          "%s step %d atom %d" % (label, k, a)):
                    failed[a].append(k)
                if not fin[a]:
                    written[a].add(int(after[a]["state"][3]))
                H = int(after[a]["state"][4])
                rec.append([after[a]["state"].copy(), after[a]["gamma"].copy(), after[a]["slab"][:, :M.n_dots(H)].copy(),
                            after[a]["ring"][:, sorted(written[a])][..., 1:].copy()] + [v.copy() for v in row(got) if v is not None])
            records.append(rec)
            before = after
        if checked:
            print(worst.line(label))
            assert worst.neg > 0, (label, "no clearly negative candidate: the clamp's test is vacuous")
            assert worst.band <= 1e-3 * worst.nodes, (label, worst.band, worst.nodes)
    finally:
        mix.close()
        linear.close()
    return worst, failed, records


def seeded(G, lsda, seed):
    return lambda a, k: M.generate(G[1], lsda, seed, k) + (0,)


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
@pytest.mark.parametrize("N", sorted(M.LOG_GRIDS))
def test_chunk_edges(ctx, grids, N, lsda):
    """257: one partly filled chunk (node 256 is thread 0's second node); 1025: a last chunk of the single node 1024; 3 / 5 / 17 chunks;
    m = 4, warmup = 3, 13 steps: the ring wraps, under LSDA too"""
    G = grids(N)
    w, _, _ = run_case(ctx, G, lsda, 1, 4, 3, 3 + 2 * 4 + 2, seeded(G, lsda, N % 7 + 4), "N %d %s m 4" % (N, "LSDA" if lsda else "LDA"))
    assert w.accelerated == 10 and w.failed == 0


@pytest.mark.parametrize("m", range(1, 9))
def test_every_history_length(ctx, grids, m):
    """N = 1025, LSDA, warmup = 1, 2 m + 3 steps: gram_chunk<H> for H = 1 .. m, then the ring wraps; the H = 1 shift check"""
    G = grids(1025)
    w, _, _ = run_case(ctx, G, True, 1, m, 1, 1 + 2 * m + 2, seeded(G, True, 1025 % 7 + m), "N 1025 LSDA m %d" % m)
    assert w.accelerated == 2 * m + 2 and w.failed == 0 and w.shift > 0


def test_uniform_grid(ctx, grids):
    """hstep = h and cnst = 1 in the weight"""
    G = grids(1025, True)
    w, _, _ = run_case(ctx, G, False, 1, 3, 3, 3 + 2 * 3 + 2, seeded(G, False, 1025 % 7 + 3), "N 1025 LDA m 3 uniform")
    assert w.accelerated == 8 and w.failed == 0


def batch_inputs(G, lsda):
    return lambda a, k: M.batch_input(G[1], lsda, a, k)


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
def test_batch_of_atoms_in_different_phases(ctx, grids, lsda):
    """five atoms whose rings differ in head, length and pairs in use: one frozen from step 6, one whose step 2 repeats step 1 (trace 0,
    first pivot 0), one with a NaN node at step 7 and an Inf node at step 11.  The failed solves are the designed behaviour: the
    linear step, the history cleared, everything finite elsewhere -- all asserted by check_step -- on exactly the planned steps"""
    G = grids(1025)
    w, failed, rec = run_case(ctx, G, lsda, M.BATCH_ATOMS, M.BATCH_M, M.BATCH_WARMUP, M.BATCH_STEPS, batch_inputs(G, lsda),
                              "batch of 5, N 1025 %s m 3" % ("LSDA" if lsda else "LDA"))
    assert failed == M.BATCH_FAILURES, failed
    states = [[int(v) for v in rec[-1][a][0][:3]] for a in range(M.BATCH_ATOMS)]
    assert states[1] == [2, 3, 5] and states[0] == [14 % 3, 3, 14] and states[2] == [12 % 3, 3, 14] and states[3] == [0, 3, 14], states
    assert len({tuple(rec[9][a][0][:6]) for a in range(M.BATCH_ATOMS)}) >= 4          # step 10: neighbours in different phases


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
def test_batch_independence_and_run_to_run_identity(ctx, grids, lsda):
    """the same batch twice, and each atom alone: slab, gamma, state, ring and outputs bit for bit"""
    G = grids(1025)
    inp = batch_inputs(G, lsda)
    args = (M.BATCH_M, M.BATCH_WARMUP, M.BATCH_STEPS)
    first = run_case(ctx, G, lsda, M.BATCH_ATOMS, *args, inp, "", checked=False)[2]
    again = run_case(ctx, G, lsda, M.BATCH_ATOMS, *args, inp, "", checked=False)[2]
    for a in range(M.BATCH_ATOMS):
        alone = run_case(ctx, G, lsda, 1, *args, lambda _, k, a=a: inp(a, k), "", checked=False)[2]
        for k in range(M.BATCH_STEPS):
            for n, (u, v, t) in enumerate(zip(first[k][a], again[k][a], alone[k][0])):
                assert u.shape == v.shape == t.shape and (np.array_equal(u, v) and np.array_equal(u, t) if n == 0 else same(u, v) and same(u, t)), (a, k + 1, n)


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
def test_duplicate_pair(ctx, grids, lsda):
    """m = 2, warmup = 2, steps 1 and 2 with the same input: step 3 solves the regularised singular system (d of the module docstring);
    |gamma_0 + gamma_1 - exact| / (eps |exact|) of the float64 reference on the model's dots: 0.14 (LDA), 0.12 (LSDA); the device's: not
    yet measured (see the module docstring)"""
    G = grids(1025)
    grid, r = G[0], G[1]
    w, failed, rec = run_case(ctx, G, lsda, 1, M.DUP_M, M.DUP_WARMUP, M.DUP_STEPS, lambda a, k: M.dup_input(r, lsda, k) + (0,),
                              "duplicate pair N 1025 %s" % ("LSDA" if lsda else "LDA"))
    assert not failed[0] and w.accelerated == 3
    state, gamma, slab = rec[2][0][:3]
    assert state.tolist()[3:6] == [0, 2, 1] and np.all(np.isfinite(gamma))
    dots = np.zeros(5)
    for c in range(slab.shape[0]):
        dots = dots + slab[c]
    A, b = M.unpack(dots, 2)
    assert A[0, 0] == A[0, 1] == A[1, 1] > 0 and b[0] == b[1], (A, b)
    Ar, lam = M.regularised(A)
    exact = 2 * LD(b[0]) / (2 * LD(A[0, 0]) + LD(lam))
    ref = AR.cholesky_solve(Ar, b)
    d_ref = abs(LD(ref[0]) + LD(ref[1]) - exact)
    d_dev = abs(LD(gamma[0]) + LD(gamma[1]) - exact)
    print("duplicate pair %s: gamma device %s reference %s; |gamma_0 + gamma_1 - exact| / (eps |exact|): reference %.3f, device %.3f"
          % ("LSDA" if lsda else "LDA", gamma[:2], ref, float(d_ref / (EPS * abs(exact))), float(d_dev / (EPS * abs(exact)))))
    assert d_dev <= 8 * d_ref, (float(d_dev), float(d_ref))
