"""Electron configurations (no GPU needed): dfta_config_parse / dfta_ion_config, the host code behind Scf(config=..., charge=...).
Level arrays count n as get_subshells does (principal quantum number - 1); the text uses the principal quantum number.

Charge 0 must give exactly the arrays of the Aufbau path (dfta_get_subshells_ex / dfta_split_spin_ex), so that a neutral atom
built from a configuration runs the same levels with the same occupations as the default path.
"""
import ctypes as C

import numpy as np
import pytest

import dftatom_amd as D


def _aufbau(Z, lsda, aufbau):
    lib = D.load()
    n, l, o, bn, bl, bo = (np.zeros(32, np.int32) for _ in range(6))
    if not lsda:
        cnt = lib.dfta_get_subshells_ex(Z, aufbau, D._ip(n), D._ip(l), D._ip(o), 32)
        return {"alpha": [(int(n[k]), int(l[k]), float(o[k])) for k in range(cnt)], "beta": []}
    nA, nB = C.c_int(), C.c_int()
    assert lib.dfta_split_spin_ex(Z, aufbau, C.byref(nA), C.byref(nB), D._ip(n), D._ip(l), D._ip(o), D._ip(bn), D._ip(bl), D._ip(bo), 32) == 0
    return {"alpha": [(int(n[k]), int(l[k]), float(o[k])) for k in range(nA.value)],
            "beta": [(int(bn[k]), int(bl[k]), float(bo[k])) for k in range(nB.value)]}


def _text(cfg_lda):
    return " ".join("%d%s%g" % (n + 1, "spdf"[l], o) for n, l, o in cfg_lda["alpha"])


@pytest.mark.parametrize("aufbau", [D.AUFBAU_REFERENCE, D.AUFBAU_TRANSITION_METALS])
@pytest.mark.parametrize("lsda", [False, True])
def test_charge_zero_is_the_aufbau_configuration(lsda, aufbau):
    for Z in range(1, 119):
        assert D.ion_config(Z, 0, lsda, aufbau) == _aufbau(Z, lsda, aufbau), Z


@pytest.mark.parametrize("aufbau", [D.AUFBAU_REFERENCE, D.AUFBAU_TRANSITION_METALS])
@pytest.mark.parametrize("lsda", [False, True])
def test_aufbau_text_parses_to_the_aufbau_configuration(lsda, aufbau):
    for Z in range(1, 119):
        text = _text(_aufbau(Z, False, aufbau))
        assert D.parse_config(Z, text, lsda, aufbau) == _aufbau(Z, lsda, aufbau), (Z, text)


@pytest.mark.parametrize("lsda", [False, True])
def test_charge_conserves_electrons(lsda):
    for Z in range(1, 119):
        for q in (1, 2, 3):
            if q >= Z:
                with pytest.raises(D.DftaError):
                    D.ion_config(Z, q, lsda)
                continue
            assert D.config_electrons(D.ion_config(Z, q, lsda)) == Z - q, (Z, q)


def test_charge_rule_examples():
    assert D.ion_config(26, 1) == {"alpha": [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0), (2, 0, 2.0), (2, 1, 6.0), (2, 2, 6.0), (3, 0, 1.0)],
                                   "beta": []}                                              # Fe+ = [Ar] 3d6 4s1
    assert D.ion_config(26, 2)["alpha"][-1] == (2, 2, 6.0)                                   # Fe2+ = [Ar] 3d6
    ar = D.ion_config(18, 1, lsda=True)                                                      # Ar+ LSDA: 3p 3/2
    assert (2, 1, 3.0) in ar["alpha"] and (2, 1, 2.0) in ar["beta"]
    assert D.ion_config(11, 1) == D.parse_config(11, "[He] 2s2 2p6")                        # Na+ = [Ne]
    assert D.ion_config(3, 1, lsda=True) == {"alpha": [(0, 0, 1.0)], "beta": [(0, 0, 1.0)]}


def test_fractional_and_core_tokens():
    cfg = D.parse_config(18, "[Ne] 3s2 3p5.5")
    assert cfg == {"alpha": [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0), (2, 0, 2.0), (2, 1, 5.5)], "beta": []}
    cfg = D.parse_config(18, "[Ne] 3s2 3p5.5", lsda=True)
    assert (2, 1, 3.0) in cfg["alpha"] and (2, 1, 2.5) in cfg["beta"]
    cfg = D.parse_config(7, "[He] 2s2 2p2/1", lsda=True)                                    # explicit split
    assert cfg["alpha"][-1] == (1, 1, 2.0) and cfg["beta"][-1] == (1, 1, 1.0)
    assert D.parse_config(10, "[Ne] 2p5 3s1") == {"alpha": [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 5.0), (2, 0, 1.0)], "beta": []}
    assert D.parse_config(10, "[Ne] 2s0") == {"alpha": [(0, 0, 2.0), (1, 1, 6.0)], "beta": []}   # 0 removes a core subshell
    assert D.parse_config(3, "2p1 1s2") == {"alpha": [(0, 0, 2.0), (1, 1, 1.0)], "beta": []}      # sorted by (n, l)
    assert D.config_electrons(D.parse_config(18, "[Ar]")) == 18


@pytest.mark.parametrize("Z, text, lsda", [
    (10, "1s2 2s2 2p7", False),            # over-filled subshell
    (5, "1s2 2s2 2p4/0", True),            # over-filled spin channel
    (3, "1s2 1p1", False),                 # l >= n
    (20, "[Ar] 5g2", False),               # l > 3 (not a spdf letter)
    (3, "1s2 2s1 2s1", False),             # duplicate
    (10, "[Xx] 2s2", False),               # unknown core
    (9, "[Ne]", False),                    # N_e > Z: anion
    (10, "1s0", False),                    # N_e = 0
    (10, "", False),                       # nothing
    (10, "hello", False),                  # garbage
    (10, "[Ne] 3s", False),                # occupation missing
    (10, "1s2x", False),                   # trailing characters
    (10, "1s-1 [Ne]", False),              # negative occupation
    (7, "[He] 2s2 2p2/1", False),          # a spin split needs LSDA
    (0, "1s1", False),                     # Z out of range
    (119, "1s1", False),
])
def test_invalid_configurations_are_refused(Z, text, lsda):
    with pytest.raises(D.DftaError) as e:
        D.parse_config(Z, text, lsda)
    assert "invalid electron configuration: " in str(e.value) and len(str(e.value)) > 40


def test_invalid_charges_are_refused():
    for Z, q in ((18, -1), (18, 18), (1, 1), (0, 0), (119, 0)):
        with pytest.raises(D.DftaError):
            D.ion_config(Z, q)
