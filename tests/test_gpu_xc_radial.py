"""GPU suite (-m gpu): the radial XC kernels -- k_pbe_radial (gga.hip) and k_pw92_lda / k_pw92_lsda (xc.hip), through
dfta_xc_radial -- at their edges, against tests/_gga_ref.radial evaluated in EXTENDED precision (np.longdouble).

An fp64 copy of the kernel's formulas shares the kernel's rounding and cannot see it (that is how a difference stencil that lost a
factor 1 / delta to cancellation got through, see _gga_ref.d_index).  So every output (res, va, vb, eexc) is held, node by node, to

    |gpu - ref_ext|(j)  <=  8 E(j) + 1e-11 T(j)

E(j): the fp64 reference's own distance from the extended one, |ref64 - ref_ext|, as a running maximum over j-8 .. j+8 -- what
      fp64 arithmetic costs this formula on this grid at this node, measured, not chosen; the factor 8 is for the GPU's cbrt,
      log1p, expm1 differing from NumPy's;
T(j): the sum of the magnitudes of the terms the output is made of (_gga_ref.radial(scale=True)), with the pointwise test's gate
      1e-11 in front: the radial kernel cannot be asked for more than xc_point is.
Exact zeros where the contract says zeros (PBE: node 0 and total density < 1e-18; PW92, which is pointwise: total density < 1e-18),
everything finite.

The contract for a NaN density node, read from the kernels and tested here: that node writes zeros in every output.  PW92: no
other node changes a bit.  PBE: the node enters its neighbours' density stencils (nodes +-1, +-2), whose fluxes enter the
divergence stencils two nodes further, so the eight nodes within 4 of it are unspecified (NaN in practice); every node further
away keeps the bits of the run without the NaN.

Observed maxima of |gpu - ref_ext| / (8 E + 1e-11 T) on an MI355X (every test prints its own), PBE at 16 385 / 131 073 /
1 048 577 nodes: edges 0.014 / 0.15 / 0.35, edges_lda 0.012 / 0.15 / -, other 0.009 / 0.12 / -, gaps_lda 0.012 / 0.15 / 0.35,
gaps 0.015 / 0.21 / -, gaps_b 0.031 / 0.15 / -, empty_b 0.23 / 0.22 / -, crossing_b 0.16 / 0.20 / 0.46; batch rows as the single
rows.  PW92: crossing_b 0.13 / 0.15 / 0.21 (uniform grid 0.17), every other case below 5e-4 (there 1e-11 T is the whole gate).
With the stencils summed value by value (the library's earlier form) the fp64 reference itself misses this gate by a factor 5 to
15 at 16 385 nodes already.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _gga_ref as R                     # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD = np.longdouble
GRIDS = {"L14": (14, 5e-4, 25.0), "L17": (17, 1e-4, 50.0), "L20": (20, 1.25e-5, 50.0)}      # tests/golden/l20_meta.json
TILE = 252                               # outputs per workgroup of k_pbe_radial


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


_grids = {}


@pytest.fixture(scope="module")
def grids(ctx):
    def get(name):
        if name not in _grids:
            g = D.Grid(ctx, *GRIDS[name]) if name in GRIDS else D.Grid(ctx, 14, None, 25.0)
            if name in GRIDS:
                cnst = g.Rp * g.delta * np.exp(g.delta * np.arange(g.N, dtype=float))
            else:
                cnst = np.ones(g.N)
            _grids[name] = (g, g.r(), cnst)
        return _grids[name]
    yield get
    for g, _, _ in _grids.values():
        g.close()
    _grids.clear()


# ---- densities ---------------------------------------------------------------------------------------------------------------
def shells(r, z1=9.64, z2=2.88, tail=1e-3):
    """Slater 1s + n=2 shells and a slowly decaying tail: far above the threshold at nodes 1, 2 and N-2, N-1"""
    return (2.0 * z1 ** 3 / np.pi * np.exp(-2.0 * z1 * r) + 8.0 * (2.0 * z2) ** 5 * r * r * np.exp(-2.0 * z2 * r) / (96.0 * np.pi)
            + tail / (1.0 + r) ** 4)


def gap_nodes(N):
    """stretches of dead nodes in the middle of the grid whose ends sit on and next to tile boundaries (252 k - 2 .. 252 k + 2)"""
    nt = (N + TILE - 1) // TILE
    out = []
    for n, (d0, d1) in enumerate([(-2, 2), (-1, 1), (0, 0), (1, -1), (2, -2), (0, -1), (-1, 0)]):
        k0 = 3 + n * max(1, (nt - 8) // 8)
        k1 = k0 + 1 + n % 2                           # one or two tiles long: a tile that is dead throughout as well
        out.append((TILE * k0 + d0, TILE * k1 + d1))
    out.append((TILE * (nt - 1) - 1, TILE * (nt - 1) + 1))          # across the boundary of the partial last tile
    return out


def with_gaps(rho):
    """exact zeros, 1e-19 (below the threshold, not zero) and -0.0 alternate inside the stretches"""
    rho = rho.copy()
    for a, b in gap_nodes(rho.size):
        rho[a:b] = np.resize([0.0, 1e-19, 3e-19, -0.0], b - a)
    return rho


def density(name, r):
    """(na, nb) -- nb None: the LDA entry"""
    s = shells(r)
    if name == "edges":                # LSDA, both channels live everywhere
        return 0.55 * s, 0.45 * s
    if name == "edges_lda":
        return s, None
    if name == "other":                # another shape: Ar-like exponents, a heavier tail, a different split
        t = shells(r, 17.5, 6.1, 3e-2) + 0.3 * r ** 4 * np.exp(-2.1 * r)
        return 0.5 * t, 0.5 * t
    if name == "gaps_lda":
        return with_gaps(s), None
    if name == "gaps":                 # the total density dead in the stretches
        return with_gaps(0.6 * s), with_gaps(0.4 * s)
    if name == "empty_b":              # hydrogen-like: zeta pinned to +1 everywhere
        return s, np.zeros_like(s)
    if name == "crossing_b":           # rho_b drops below the threshold inside the grid, smoothly: positive below it, then 0
        return 0.55 * s, 0.45 * s * np.exp(-(r / 0.9) ** 2)
    if name == "gaps_b":               # rho_b dead in stretches next to tile boundaries, rho_a live throughout
        return 0.55 * s, with_gaps(0.45 * s)
    if name == "zeros":
        return np.zeros_like(s), np.zeros_like(s)
    raise KeyError(name)


# ---- the measure -------------------------------------------------------------------------------------------------------------
running_max = R.running_max


_refs = {}


def reference(functional, gname, r, cnst, dname):
    """(ref_ext, E, T) per output, cached for the module"""
    key = (functional, gname, dname)
    if key not in _refs:
        na, nb = density(dname, r)
        ext, T = R.radial(functional, r, cnst, na.astype(LD), None if nb is None else nb.astype(LD), scale=True)
        f64 = R.radial(functional, r, cnst, na, nb)
        assert all(x.dtype == LD for x in ext) and all(x.dtype == np.float64 for x in f64)
        _refs[key] = (ext, [running_max(np.abs(a - b)) for a, b in zip(f64, ext)], T)
    return _refs[key]


def check(functional, got, ref, na, nb, label):
    """the module docstring's assertions; returns (and prints) the largest |gpu - ref_ext| / (8 E + 1e-11 T)"""
    ext, E, T = ref
    rho = na if nb is None else na + nb
    dead = rho < 1e-18
    if functional == D.XC_PBE:
        dead[0] = True
    worst = 0.0
    names = ("Vexc", "eexc") if nb is None else ("res", "va", "vb", "eexc")
    for name, g, w, e, t in zip(names, got, ext, E, T):
        assert np.all(np.isfinite(g)), (label, name)
        assert np.all(g[dead] == 0.0), (label, name)
        assert np.all(w[dead] == 0.0)
        err = np.abs(g.astype(LD) - w)
        bound = 8.0 * e + 1e-11 * t
        live = ~dead
        ratio = float(np.max(err[live] / bound[live])) if live.any() else 0.0
        j = int(np.argmax(np.where(live, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print("%-40s %-5s max |gpu - ref_ext| / (8 E + 1e-11 T) = %.3f at node %d" % (label, name, ratio, j))
        assert np.all(err[live] <= bound[live]), (label, name, ratio, j)
        worst = max(worst, ratio)
    return worst


def run(ctx, grids, functional, gname, dname):
    g, r, cnst = grids(gname)
    na, nb = density(dname, r)
    got = D.xc_radial(ctx, g, functional, na, nb)
    ref = reference(functional, gname, r, cnst, dname)
    check(functional, got, ref, na, nb, "%s %s %s" % ("PBE" if functional == D.XC_PBE else "PW92", gname, dname))
    return got


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


CASES = [(g, d) for g in ("L14", "L17") for d in ("edges", "edges_lda", "other", "gaps_lda", "gaps", "empty_b", "crossing_b", "gaps_b")]
CASES += [("L20", "edges"), ("L20", "gaps_lda"), ("L20", "crossing_b")]


@pytest.mark.parametrize("functional", [D.XC_PBE, D.XC_PW92], ids=["pbe", "pw92"])
@pytest.mark.parametrize("gname,dname", CASES)
def test_single_row_against_extended_reference(ctx, grids, functional, gname, dname):
    """one atom per call on the three grids: one-sided stencils with live values (edges), dead stretches whose ends sit on and
    beside tile boundaries, an empty / a vanishing / a locally dead minority channel"""
    g, r, _ = grids(gname)
    na, nb = density(dname, r)
    if dname.startswith("edges"):
        assert min(na[1], na[2], na[-2], na[-1]) > 1e-12
    if "gaps" in dname:
        d = (na if nb is None else nb) < 1e-18
        assert d[1:-1].any() and not d[[1, 2, -2, -1]].any() and d[TILE * 3 - 2] and not d[TILE * 3 - 3]
    if dname == "crossing_b":
        d = nb < 1e-18
        assert d.any() and not d[:1000].any() and np.any(d & (nb > 0))
    run(ctx, grids, functional, gname, dname)


ROWS = ("edges", "other", "zeros", "edges", "gaps")


@pytest.mark.parametrize("functional", [D.XC_PBE, D.XC_PW92], ids=["pbe", "pw92"])
@pytest.mark.parametrize("gname,pol", [("L14", True), ("L14", False), ("L17", True), ("L20", True)])
def test_batch_rows(ctx, grids, functional, gname, pol):
    """several atoms per call (blockIdx.y, base = a N): every row against the reference, row 3 (a copy of row 0) and every other
    row bit for bit what the same row gives alone, the all-zero row zeros"""
    g, r, cnst = grids(gname)
    rows = ROWS if gname != "L20" else ("edges", "zeros", "edges")
    dens = [density(d, r) for d in rows]
    A = np.stack([d[0] for d in dens])
    B = np.stack([d[1] for d in dens])
    if not pol:
        A, B = A + B, None
    got = D.xc_radial(ctx, g, functional, A, B)
    for k, d in enumerate(rows):
        row = [x[k] for x in got]
        alone = D.xc_radial(ctx, g, functional, A[k], None if B is None else B[k])
        for x, y in zip(row, alone):
            assert np.array_equal(bits(x), bits(y)), (gname, k, d)
        if d == "zeros":
            assert all(np.all(x == 0.0) for x in row)
        elif pol:
            check(functional, row, reference(functional, gname, r, cnst, d), A[k], B[k], "batch %s row %d %s" % (gname, k, d))
    for x in got:
        assert np.array_equal(bits(x[rows.index("edges")]), bits(x[len(rows) - 1 if gname == "L20" else 3]))
    if not pol:                                     # the LDA rows: the sums of the LSDA cases' channels, checked on their own
        na = A[1]
        ext, T = R.radial(functional, r, cnst, na.astype(LD), scale=True)
        f64 = R.radial(functional, r, cnst, na)
        ref = (ext, [running_max(np.abs(a - b)) for a, b in zip(f64, ext)], T)
        check(functional, [x[1] for x in got], ref, na, None, "batch %s row 1 other (LDA)" % gname)


@pytest.mark.parametrize("functional", [D.XC_PBE, D.XC_PW92], ids=["pbe", "pw92"])
@pytest.mark.parametrize("gname", ["L14", "L17"])
@pytest.mark.parametrize("dname", ["edges", "crossing_b", "gaps_b", "empty_b"])
def test_spin_exchange_exchanges_bits(ctx, grids, functional, gname, dname):
    """rho_a <-> rho_b: res and eexc keep their bits, va and vb exchange theirs (zeta = -1 pinned included)"""
    g, r, _ = grids(gname)
    na, nb = density(dname, r)
    res, va, vb, ee = D.xc_radial(ctx, g, functional, na, nb)
    res2, va2, vb2, ee2 = D.xc_radial(ctx, g, functional, nb, na)
    for x, y, n in ((res, res2, "res"), (va, vb2, "va"), (vb, va2, "vb"), (ee, ee2, "eexc")):
        assert np.array_equal(bits(x), bits(y)), (n, int(np.sum(bits(x) != bits(y))))
    assert np.any(va != vb)


@pytest.mark.parametrize("pol", [False, True], ids=["lda", "lsda"])
@pytest.mark.parametrize("functional", [D.XC_PBE, D.XC_PW92], ids=["pbe", "pw92"])
def test_nan_node(ctx, grids, functional, pol):
    """the contract of the module docstring, with the NaN inside a tile, on a tile boundary and (LSDA) in the minority channel"""
    g, r, _ = grids("L14")
    na, nb = density("edges", r)
    if not pol:
        na, nb = na + nb, None
    clean = D.xc_radial(ctx, g, functional, na, nb)
    for node, chan in ((1000, 0), (TILE * 7, 0), (TILE * 9 - 1, 1), (g.N - 3, 0)):
        a, b = na.copy(), None if nb is None else nb.copy()
        (b if (chan and pol) else a)[node] = np.nan
        got = D.xc_radial(ctx, g, functional, a, b)
        far = np.abs(np.arange(g.N) - node) > (4 if functional == D.XC_PBE else 0)
        for x, y in zip(got, clean):
            assert x[node] == 0.0
            assert np.array_equal(bits(x[far]), bits(y[far])), (node, chan)
            assert np.all(np.isfinite(x[far]))


@pytest.mark.parametrize("pol", [False, True], ids=["lda", "lsda"])
def test_pw92_uniform_grid(ctx, grids, pol):
    """k_pw92_* have no grid dependence and the entry point takes the uniform grid: same measure; node 0 is a node like any other"""
    g, r, cnst = grids("uniform")
    assert g.N == 16385 and abs(r[1] - 25.0 / 16384) < 1e-15
    for dname in ("edges", "gaps", "crossing_b"):
        na, nb = density(dname, r)
        if not pol:
            na, nb = na + nb, None
        got = D.xc_radial(ctx, g, D.XC_PW92, na, nb)
        ext, T = R.radial(R.PW92, r, cnst, na.astype(LD), None if nb is None else nb.astype(LD), scale=True)
        f64 = R.radial(R.PW92, r, cnst, na, nb)
        ref = (ext, [running_max(np.abs(x - y)) for x, y in zip(f64, ext)], T)
        check(D.XC_PW92, got, ref, na, nb, "PW92 uniform %s %s" % (dname, "lsda" if pol else "lda"))
        assert got[0][0] != 0.0 and got[0][0] == D.xc_radial(ctx, g, D.XC_PW92, np.roll(na, 1), None if nb is None else np.roll(nb, 1))[0][1]
