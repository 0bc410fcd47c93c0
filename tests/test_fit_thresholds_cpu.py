"""Proof on the CPU that the inputs of test_gpu_fit_thresholds.py bite (no GPU, no engine).

For every batch of that suite: the coverage conditions hold on its threshold inventory (every node rank of every
dimension, a knife pair at every value, the label knives), the numpy reference equals the C oracle, the unmutated
emulators of fit_encodings.py equal the reference -- and every mutant of every emulator differs from the reference on
a named case.  Flip a switch of fit_encodings.MUTANTS into the unmutated call below and the exactness test fails on
the threshold inventory; the same mutants over the inventories of the earlier fit tests are recorded (not asserted)
in DESIGN.md section 26."""
import numpy as np
import pytest

import fit_encodings as FE
import fit_thresholds as FT
import oracle

SWEEP = {"sweep_2": (2, (0, 0, 0)), "sweep_3": (3, (0, 0, 0)), "sweep_4": (4, (0, 0, 0)), "sweep_64": (64, (0, 0, 0)),
         "sweep_12_pressed": (12, (0, 0, 145)), "sweep_252_pressed": (252, (45, 45, 44))}   # (m, ballast)


def _cases():
    out = {k: v + (FT.build_inventory(*v, seed=3 + i, n_diag=2000 if k == "adversarial" else 400),)
           for i, (k, v) in enumerate(FT.path_batches().items())}
    for name in list(FT.CODED_SEAMS) + list(FT.PLANE_SEAMS):
        req, need = FT.seam_batch(name)
        out[name] = (req, need, FT.seam_inventory(name, req, need))
    for s, kind in FT.I32_SEAMS:
        out[f"i32_{kind}_s{s}"] = FT.i32_case(s, kind)
    for name, (m, ballast) in SWEEP.items():
        req, need = FT.sweep_batch(m, ballast)
        out[name] = (req, need, FT.build_inventory(req, need, seed=m, n_diag=50))
    return out


NAMES = list(_cases())


@pytest.fixture(scope="module")
def cases():
    """name -> (req, need, inventory, residuals and labels with the removable slots gone, reference rows)."""
    out = {}
    for k, (req, need, inv) in _cases().items():
        res, lab = inv.reference()
        out[k] = (req, need, inv, res, lab, FT.fit_rows(res, lab, req, need))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_inventory_covers_the_batch(cases, name):
    req, need, inv, res, lab, want = cases[name]
    assert (inv.cap >= 0).all() and (inv.used >= 0).all() and inv.cap.shape[1] % 64
    np.testing.assert_array_equal(inv.cap - inv.used, inv.residual())
    FT.assert_covered(FT.coverage(res, lab, req, need), name)
    if name in FT.CODED_SEAMS or name in FT.PLANE_SEAMS:                 # the value tables
        ks = (FT.CODED_SEAMS.get(name) or FT.PLANE_SEAMS[name])[0]
        assert tuple(len(np.unique(req[:, d])) for d in range(4)) == ks
        assert (len(req) - 1) % 16 and (req[:, 0] == 0).any() and req.min() >= 0
        for f in range(4):
            if ks[f] >= 6:
                assert set(FT.SPECIAL_VALUES) <= set(req[:, f].tolist())
    if name == "int64max":
        assert req[:, 1].max() == FT.I64MAX


@pytest.mark.parametrize("name", NAMES)
def test_references_agree(cases, name):
    req, need, inv, res, lab, want = cases[name]
    rows, counts = FT.fit_packed(res, lab, req, need, cells=1 << 22)     # (several bands of jobs)
    o_mask, o_counts = oracle.fit_mask(res, lab, req, need)
    np.testing.assert_array_equal(rows, o_mask)
    np.testing.assert_array_equal(counts, o_counts)
    np.testing.assert_array_equal(rows, FT.pack_rows(want))
    assert 0 < counts.sum() < want.size


def emulations(name, req, need, res, lab):
    """(what, rows) of every unmutated emulator that takes the batch."""
    for L in (2, 3) if name == "adversarial" else (1, 2, 3, 4):
        yield f"digit planes L {L}", FE.lds_fit(res, lab, req, need, levels=L)
    if name == "many":
        for B in (2, 3, 7):
            yield f"digit planes L 3 B {B}", FE.lds_fit(res, lab, req, need, levels=3, base=B)
    got = FE.i32_fit(res, lab, req, need)
    if got is not None:
        yield "int32", got
    for no_therm in (False, True):
        got = FE.coded_fit(res, lab, req, need, no_therm=no_therm)
        if got is not None:
            yield f"coded no_therm {no_therm}", got


@pytest.mark.parametrize("name", NAMES)
def test_emulators_are_exact(cases, name):
    req, need, inv, res, lab, want = cases[name]
    for what, got in emulations(name, req, need, res, lab):
        bad = np.argwhere(got != want)
        assert not len(bad), (name, what, len(bad), bad[:4].tolist())


def test_which_batches_the_emulators_take(cases):
    """The int32 and coded emulators refuse what the builders refuse (and only that)."""
    for name, (req, need, *_) in cases.items():
        if name.startswith("i32_"):
            assert (FE.i32_shifts(req) is None) == ("odd" in name), name
            if "odd" not in name:
                s = int(name.rsplit("s", 1)[1]) + ("over" in name)
                assert FE.i32_shifts(req) == [s] * 4, name
    plan = {k: FE.coded_plan(*FT.CODED_SEAMS[k]) for k in FT.CODED_SEAMS}
    swar = {k: FE.coded_plan(*FT.CODED_SEAMS[k], no_therm=True) for k in FT.CODED_SEAMS}
    assert plan["therm31"][0] and not plan["therm32"][0] and swar["therm31"] == (False, [5, 5, 4, 4, 3])
    for k, b in (("swar_k3", 3), ("swar_k4", 4), ("swar_k7", 4), ("swar_k8", 5)):
        assert swar[k][1][0] == b, k
    assert swar["swar_k15"][1][1] == 5 and swar["swar_k16"][1][1] == 6
    assert swar["swar_k127"][1][0] == 8 and swar["swar_k128"] is None and plan["swar_k128"] is None
    assert sum(swar["word32"][1]) == 32 and swar["word33"] is None
    assert swar["needs4"][1][4] == 4 and swar["antichain"] is None and plan["antichain"] is None
    for k, (ks, needs) in FT.PLANE_SEAMS.items():
        assert (sum(ks) + len(needs) <= 32) == k.startswith("pairs32"), k
    sizes = {k: FE.plane_set_sizes(*cases[k][:2]) for k in FT.PLANE_SEAMS if not k.startswith("pairs32")}
    assert sizes["pairs33"] == [(32, 33), (5, None)]
    assert sizes["sets_close_at_31"][0] == (31, 33)
    assert sizes["sets_full_twice"] == [(32, 33), (32, 33), (5, None)]


# (mutant, the named case that catches it, the emulation)
CAUGHT = [
    ("top_short", "adversarial", lambda a, mu: FE.lds_fit(*a, levels=2, mutant=mu)),
    ("top_short", "sweep_64", lambda a, mu: FE.lds_fit(*a, levels=3, mutant=mu)),
    ("ge_c", "adversarial", lambda a, mu: FE.lds_fit(*a, levels=2, mutant=mu)),
    ("ge_c", "many", lambda a, mu: FE.lds_fit(*a, levels=3, mutant=mu)),
    ("base_off", "many", lambda a, mu: FE.lds_fit(*a, levels=1, mutant=mu)),
    ("base_off", "sweep_2", lambda a, mu: FE.lds_fit(*a, levels=2, mutant=mu)),
    ("rank_lower", "adversarial", lambda a, mu: FE.lds_fit(*a, levels=3, mutant=mu)),
    ("rank_lower", "sweep_3", lambda a, mu: FE.lds_fit(*a, levels=1, mutant=mu)),
    ("round_zero", "i32_over_s6", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("round_zero", "i32_over_s0", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("neg_zero", "i32_max_s0", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("neg_zero", "cfg5", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("sat_low", "i32_max_s6", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("sat_low", "i32_max_s0", lambda a, mu: FE.i32_fit(*a, mutant=mu)),
    ("narrow", "swar_k8", lambda a, mu: FE.coded_fit(*a, no_therm=True, mutant=mu)),
    ("narrow", "swar_k16", lambda a, mu: FE.coded_fit(*a, no_therm=True, mutant=mu)),
    ("narrow", "needs4", lambda a, mu: FE.coded_fit(*a, no_therm=True, mutant=mu)),
    ("therm_no_minus", "therm31", lambda a, mu: FE.coded_fit(*a, mutant=mu)),
    ("therm_no_minus", "chain", lambda a, mu: FE.coded_fit(*a, mutant=mu)),
]


@pytest.mark.parametrize("mutant,name,fn", CAUGHT, ids=[f"{m}-{n}" for m, n, _ in CAUGHT])
def test_mutant_is_caught(cases, mutant, name, fn):
    req, need, inv, res, lab, want = cases[name]
    got = fn((res, lab, req, need), mutant)
    assert got is not None, "the emulator does not take the batch"
    np.testing.assert_array_equal(fn((res, lab, req, need), None), want)
    assert (got != want).any(), f"{mutant} equals the reference on {name}"


def test_every_mutant_has_a_case():
    assert {m for m, _, _ in CAUGHT} == {m for ms in FE.MUTANTS.values() for m in ms}
