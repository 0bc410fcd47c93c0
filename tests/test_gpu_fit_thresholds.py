"""The comparison itself on every fit route: nodes on both sides of every request value (fit_thresholds.py).

Every case builds its inventory FROM its batch -- knife nodes at v - 1, v, v + 1 of every value of every dimension,
diagonal nodes, label knives, INT64 extremes, negative residuals and two removed slots, shuffled, N no multiple of
64 -- forces its kernel through pe_config.fit_path_mask (and PE_LDS_W / PE_LDS_MAXL, set and restored around the
call), asserts that the path's stats counter moves by one, and compares pe_fit_mask_rows and the counts bit for bit
with fit_thresholds.fit_rows (numpy int64 comparisons).  test_fit_thresholds_cpu.py shows on the CPU that these
inputs reach every node rank and that encodings wrong by one rank, digit or bit differ on them.

The ten routes are the keys of test_gpu_mask_device.PATHS (test_every_path_on_its_threshold_inventory runs each and
asserts its counter); digit levels 1 to 3 are asserted from the PE_LDS_DEBUG plan lines at every block size in the
level sweeps, level 4 (block sizes 2 and 4 only) in test_lds_four_levels_on_digit_boundaries."""
import contextlib
import os

import numpy as np
import pytest

import fit_encodings as FE
import fit_thresholds as FT
from placement import PE_NODE_REMOVE, Engine, synth
from test_gpu_mask_device import PATHS, RUNS

pytestmark = pytest.mark.gpu

LDS_BUDGET = {1: 640, 2: 320, 4: 160}       # planes a block of 2048 W nodes holds in 160 KiB of LDS


@contextlib.contextmanager
def environ(**kv):
    kv = {k: str(v) for k, v in kv.items() if v is not None}
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    """One context per fit_path_mask for the whole module."""
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Engine(0, fit_path_mask=bits)
        return made[bits]

    yield get
    for e in made.values():
        e.close()


def counted(e, stat, extra, fn, *args, W=None, maxl=None, debug=None, cross=None):
    """fn(*args) is exactly one run of the kernel that counts in `stat`."""
    s0 = e.stats()
    with environ(PE_LDS_W=W, PE_LDS_MAXL=maxl, PE_LDS_DEBUG=debug, PE_LDS_CROSS=cross):
        out = fn(*args)
    s1 = e.stats()
    d = {k: s1[k] - s0[k] for k in s1}
    assert d[stat] == 1 and sum(d[k] for k in RUNS) == 1, (stat, {k: d[k] for k in RUNS})
    for k, v in extra.items():
        assert d[k] == v, (k, d[k], v)
    return out


def load(e, inv):
    """The inventory with its two removable slots removed; (res, labels) as the engine now holds them."""
    e.load_nodes(*inv.arrays())
    e.update_nodes(inv.remove, np.full(len(inv.remove), PE_NODE_REMOVE, np.uint8))
    return inv.reference()


def check(e, res, lab, req, need, counts=None):
    rows, want = FT.fit_packed(res, lab, req, need)
    got = e.fit_mask_rows(0, len(req))
    bad = np.argwhere(got != rows)
    assert not len(bad), f"{len(bad)} words differ, first (job, word) {bad[:4].tolist()}"
    np.testing.assert_array_equal(e.fit_counts() if counts is None else counts, want)
    return rows


def parse_plan(err):
    """The engine's last PE_LDS_DEBUG line: {"W", "cross", "fields": {dim: (m, L, B)}} (crossed fields are not
    listed: they have no digit planes)."""
    line = [ln for ln in err.splitlines() if ln.startswith("lds: W ")][-1]
    head, _, tail = line.partition("|")
    h = head.split()
    plan = {"W": int(h[h.index("W") + 1]), "cross": int(h[h.index("cross") + 1]), "fields": {}}
    t = tail.split()
    for i in range(0, len(t), 8):
        assert t[i] == "dim" and t[i + 2] == "m" and t[i + 4] == "L" and t[i + 6] == "B", line
        plan["fields"][int(t[i + 1])] = (int(t[i + 3]), int(t[i + 5]), int(t[i + 7]))
    return plan


# ---------------------------------------------------------------- a. every path on its threshold inventory

@pytest.fixture(scope="module")
def path_cases():
    """kind -> (req, need, inventory), covered (the conditions of fit_thresholds.assert_covered)."""
    out = {}
    for i, (kind, (req, need)) in enumerate(FT.path_batches().items()):
        inv = FT.build_inventory(req, need, seed=3 + i, n_diag=2000 if kind == "adversarial" else 3000)
        FT.assert_covered(FT.coverage(*inv.reference(), req, need), kind)
        out[kind] = (req, need, inv)
    return out


@pytest.mark.parametrize("path", list(PATHS))
def test_every_path_on_its_threshold_inventory(engines, path_cases, path, capfd):
    bits, stat, extra, _, kind, W = PATHS[path]
    req, need, inv = path_cases[kind]
    e = engines(bits)
    res, lab = load(e, inv)
    assert 2000 < len(lab) < 9000 and len(lab) % 64
    counts = counted(e, stat, extra, e.fit_mask, req, need, W=W, debug=1 if W else None)
    check(e, res, lab, req, need, counts)
    if W:
        assert parse_plan(capfd.readouterr().err)["W"] == W


def test_the_ten_paths():
    """Ten routes, told apart by fit_path_mask, counters and block size."""
    assert len({(v[0], v[1], tuple(sorted(v[2].items())), v[5]) for v in PATHS.values()}) == 10
    assert {v[1] for v in PATHS.values()} == set(RUNS)


# ---------------------------------------------------------------- b. LDS digit fields, dense

@pytest.mark.parametrize("W", [1, 2, 4])
def test_lds_dense_fields(engines, path_cases, W, capfd):
    """cpu, memory and ephemeral storage unique per job: 1501 node ranks in each of three digit fields."""
    req, need, inv = path_cases["adversarial"]
    e = engines(64)
    res, lab = load(e, inv)
    assert 15000 < len(lab) < 16000
    counts = counted(e, "fit_runs_lds", {}, e.fit_mask, req, need, W=W, debug=1)
    plan = parse_plan(capfd.readouterr().err)
    print("plan", plan)
    assert plan["W"] == W and all(plan["fields"][d][0] == 1500 and plan["fields"][d][1] >= 2 for d in (0, 1, 3)), plan
    check(e, res, lab, req, need, counts)


# ---------------------------------------------------------------- c. LDS level sweep

def sweep(e, capfd, W, maxl, ballast, start, stop, done, cross=None):
    """One tiny call per m = start, start + 1, ... on one context until done(seen) or stop: seen[m] = (L, B) of the
    cpu field, or None where the planner crossed it into the need planes.  ballast: a triple, or m -> a triple."""
    seen = {}
    for m in range(start, stop):
        bal = ballast(m) if callable(ballast) else ballast
        req, need = FT.sweep_batch(m, bal)
        inv = FT.build_inventory(req, need, seed=m, n_diag=20)
        if m % 8 == 4:
            FT.assert_covered(FT.coverage(*inv.reference(), req, need), f"sweep {m} {bal}")
        res, lab = load(e, inv)
        counts = counted(e, "fit_runs_lds", {}, e.fit_mask, req, need, W=W, maxl=maxl, debug=1, cross=cross)
        plan = parse_plan(capfd.readouterr().err)
        assert plan["W"] == W
        f = plan["fields"].get(0)
        assert f is None or f[0] == m
        seen[m] = f and f[1:]
        try:
            check(e, res, lab, req, need, counts)
        except AssertionError as err:
            raise AssertionError(f"W {W} PE_LDS_MAXL {maxl} m {m} ballast {bal} plan {plan}: {err}") from None
        if done(seen):
            break
    assert sorted(seen) == list(range(start, max(seen) + 1))
    return seen


def residues(seen, L):
    """Of the cases with L levels: is there one with m % B^(L-1) == 0, one with m % B^(L-1) == B^(L-1) - 1 (under
    the case's own B)?  The top level's digit count m / B^(L-1) + 2 changes between the two."""
    at = [(m, f[1] ** (L - 1)) for m, f in seen.items() if f and f[0] == L]
    return any(m % p == 0 for m, p in at), any(m % p == p - 1 for m, p in at)


def levels(seen):
    return {f[0] for f in seen.values() if f}


@pytest.mark.parametrize("W", [1, 2, 4])
def test_lds_level_sweep_one_field(engines, W, capfd):
    """One many-valued field, m = 2, 3, 4, ... (memory folded, gpu and ephemeral storage crossed), PE_LDS_MAXL 2: one
    level while the block's budget holds m planes, two past it; the sweep ends once both are seen, the two-level
    cases with m % B == B - 1.  (The planner takes the base with the fewest planes, and m / B + 2 + B grows by one
    where B divides m: on this sweep no two-level case has m % B == 0 -- the pressed sweep below reaches those.)"""
    def done(seen):
        return residues(seen, 2)[1] and 1 in levels(seen)

    seen = sweep(engines(64), capfd, W, 2, (0, 0, 0), 2, LDS_BUDGET[W] + 60, done)
    print("two-level cases", {m: f for m, f in seen.items() if f and f[0] == 2})
    assert {2, 3, 4} <= set(seen) and all(not seen[m] or seen[m][0] == 1 for m in (2, 3))     # L forced to 1 below 4
    assert levels(seen) == {1, 2} and residues(seen, 2)[1], seen


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("W", [1, 2, 4])
def test_lds_level_sweep_pressed(engines, W, L, capfd):
    """The cpu field pressed into L levels at few values, PE_LDS_MAXL = L and PE_LDS_CROSS = 0 (nothing crossed: every
    field keeps its planes).  With the cpu field alone, L levels are reached only once L - 1 overflow the block's
    budget of planes (640 / 320 / 160 at W = 1 / 2 / 4): three levels past m = 10^5 at W = 1, no tiny call, and at
    such m the planner's base never divides m.  So the other dimensions are given values that take the budget:
      L = 2: ephemeral storage budget - 3 - m values, one more than leaves room for m single-level planes; m = 2 ..:
             one level up to m = 7, two from 8, among them m = 12 in base 3 (12 % 3 == 0) and m = 8 (8 % 3 == 2);
      L = 3: memory, gpu and ephemeral storage a third of budget - 26 each: two levels of the cpu field do not fit
             beside them, three do, and two levels for one of THEM cost as many plane reads; m = 245 ..: base 6,
             among them m = 251 (251 % 36 == 35) and m = 252 (252 % 36 == 0).
    The sweep ends once L-level cases with both residues are seen; all of this is asserted from the plan lines."""
    budget = LDS_BUDGET[W]
    if L == 2:
        seen = sweep(engines(64), capfd, W, 2, lambda m: (0, 0, budget - 3 - m), 2, 40,
                     lambda seen: all(residues(seen, 2)) and 1 in levels(seen), cross=0)
        assert {2, 3, 4} <= set(seen) and all(seen[m] and seen[m][0] == 1 for m in (2, 3, 4))
        assert levels(seen) == {1, 2}, seen
    else:
        S = budget - 26
        seen = sweep(engines(64), capfd, W, 3, tuple(S // 3 + (i < S % 3) for i in range(3)), 245, 290,
                     lambda seen: all(residues(seen, 3)), cross=0)
        assert 3 in levels(seen), seen
    print("cases", seen)
    assert residues(seen, L) == (True, True), seen


# ---------------------------------------------------------------- d. four levels

@pytest.mark.parametrize("W,dims", [(2, (0, 1, 3)), (4, (0, 1))])
def test_lds_four_levels_on_digit_boundaries(engines, W, dims, capfd):
    """60 000 values unique per job in each of `dims` (the batches of test_lds_four_level_fields): the plan depends on
    the batch only, so every field's B and L (four for at least one) are read from one call over a tiny inventory;
    then 8191 nodes whose ranks lie on the digit boundaries t * B^k + {-1, 0, +1}, at both ends of the rank range and
    at random."""
    J, n = 60000, 8191
    rng = np.random.default_rng(73 + W)
    req, need = synth.make_fit_jobs(J, 73 + W)
    scale = {0: 1, 1: 1 << 20, 3: 7}
    for d in dims:
        req[:, d] = scale[d] * (1 + rng.permutation(J))
    e = engines(64)
    tiny = FT.build_inventory(req[:50], need[:50], seed=W, n_diag=10)
    load(e, tiny)
    counted(e, "fit_runs_lds", {}, e.fit_mask, req, need, W=W, debug=1)
    plan = parse_plan(capfd.readouterr().err)
    print("plan", plan)
    assert plan["W"] == W and all(plan["fields"][d][0] == J for d in dims), plan
    assert 4 in {plan["fields"][d][1] for d in dims}, plan          # (the planner may give the other fields three)
    # the nodes
    res = np.empty((4, n), dtype=np.int64)
    for d in range(4):
        vals = np.unique(req[:, d])
        if d in dims:
            _, L, B = plan["fields"][d]
            ranks = rng.permutation(FT.digit_boundary_ranks(J, B, L, 300, 2500, 79 + d))
            assert 5000 < len(ranks) <= n, len(ranks)
            ranks = np.resize(ranks, n)
            dg = FT.digits(ranks, B, L)
            for k in range(L):                    # every value the node's digit can take, at every level
                top = J // B ** k if k == L - 1 else B - 1
                assert set(dg[k].tolist()) == set(range(top + 1)), (d, k)
                # a job one step of this level above and one below: the ranks first differ at level k, both ways
                inner = (dg[k] >= 1) & (dg[k] < top) & (ranks - B ** k >= 1) & (ranks + B ** k <= J)
                assert inner.any(), (d, k)
        else:
            ranks = rng.integers(0, len(vals) + 1, n)
        res[d] = FT.residual_of_rank(vals, ranks, rng)
        np.testing.assert_array_equal(FT.node_ranks(vals, res[d]), ranks)
    lab = np.where(rng.integers(0, 4, n) > 0, np.bitwise_or.reduce(need), rng.choice(need, n)).astype(np.uint32)
    cap, used = FT.split_residual(res)
    island = np.where(lab & FT.ISLAND, np.arange(n), -1).astype(np.int32)
    e.load_nodes(cap, used, lab & ~FT.ISLAND, island)
    counts = counted(e, "fit_runs_lds", {}, e.fit_mask, req, need, W=W, debug=1)
    assert parse_plan(capfd.readouterr().err) == plan
    check(e, res, lab, req, need, counts)
    assert 0 < counts.sum() < n * J


# ---------------------------------------------------------------- e. coded seams

@pytest.mark.parametrize("bits", [5, 13])
@pytest.mark.parametrize("name", list(FT.CODED_SEAMS))
def test_coded_seams(engines, name, bits):
    """fit_path_mask 5 (the coded kernels, thermometer allowed) and 13 (thermometer refused).  The expected counter
    follows build_codes' arithmetic, restated in fit_encodings.coded_plan: a batch is coded if every field has fewer
    than CODE_MAXV = 128 values, the needs form a chain and the word fits 32 bits; a field of k values takes
    bit_length(k) + 1 bits (the ranks 0 .. k and a guard bit) -- or, if the five counts add up to at most 31 and the
    thermometer is allowed, k bits.  A batch that is not coded lands on the int64 compare (these masks leave out the
    32-bit one) and is exact all the same."""
    ks, needs = FT.CODED_SEAMS[name]
    req, need = FT.seam_batch(name)
    inv = FT.seam_inventory(name, req, need)
    plan = FE.coded_plan(ks, needs, no_therm=bool(bits & 8))
    e = engines(bits)
    res, lab = load(e, inv)
    if plan is None:
        counts = counted(e, "fit_runs_i64", {"fit_runs_therm": 0}, e.fit_mask, req, need)
    else:
        counts = counted(e, "fit_runs_coded", {"fit_runs_therm": int(plan[0])}, e.fit_mask, req, need)
    check(e, res, lab, req, need, counts)


# ---------------------------------------------------------------- f. plane seams

PLANE_RUNS = ([(k, 16, "fit_runs_planes", 0) for k in FT.PLANE_SEAMS if k.startswith("pairs32")] +
              [(k, 16 | 32, "fit_runs_planes", 0) for k in FT.PLANE_SEAMS if k.startswith("pairs32")] +
              [(k, 16, "fit_runs_planes", 1) for k in FT.PLANE_SEAMS if not k.startswith("pairs32")] +
              [(k, 0, "fit_runs_lds", 0) for k in ("pairs33", "pairs33_spread")])


@pytest.mark.parametrize("name,bits,stat,sets", PLANE_RUNS, ids=[f"{k}-{b}" for k, b, _, _ in PLANE_RUNS])
def test_plane_seams(engines, name, bits, stat, sets):
    """32 (field, value) pairs in all are one register plane set, in both layouts; 33 are plane sets where only the
    plane kernels are allowed and LDS digit planes where every path is.  fit_encodings.plane_set_sizes restates the
    sweep that fills the sets: `pairs33` and `sets_full_twice` close sets with exactly 32 planes, `sets_close_at_31`
    closes one at 31 because the next job would bring 33 (test_fit_thresholds_cpu.py asserts those sizes)."""
    ks, needs = FT.PLANE_SEAMS[name]
    assert (sum(ks) + len(needs) <= 32) == (sets == 0 and stat == "fit_runs_planes")
    req, need = FT.seam_batch(name)
    inv = FT.seam_inventory(name, req, need)
    e = engines(bits)
    res, lab = load(e, inv)
    counts = counted(e, stat, {"fit_runs_sets": sets}, e.fit_mask, req, need)
    check(e, res, lab, req, need, counts)


# ---------------------------------------------------------------- g. int32 seams

@pytest.mark.parametrize("s,kind", FT.I32_SEAMS, ids=[f"{k}-s{s}" for s, k in FT.I32_SEAMS])
def test_i32_seams(engines, s, kind):
    """fit_path_mask 3.  `max`: the largest request is INT32_MAX << s, the shift stays s and that request becomes
    INT32_MAX, the value the residuals saturate at; `over`: 2^31 << s, the shift becomes s + 1; `odd`: one request
    has a bit below that shift and the batch runs on the int64 compare.  Nodes sit on the saturation line and one
    above, with and without bits below the shift, and at -1, -2^s and -2^s - 1."""
    req, need, inv = FT.i32_case(s, kind)
    assert req.max() == (FT.I32MAX << s if kind == "max" else (1 << 31) << s)
    shifts = FE.i32_shifts(req)
    assert shifts == (None if kind == "odd" else [s + (kind == "over")] * 4)
    res_all = inv.residual()
    for v in FT.i32_nodes(s)[:, 0]:
        assert (res_all == v).all(axis=0).any(), v
    FT.assert_covered(FT.coverage(*inv.reference(), req, need), f"i32 {kind} {s}")
    e = engines(3)
    res, lab = load(e, inv)
    counts = counted(e, "fit_runs_i64" if kind == "odd" else "fit_runs_i32", {}, e.fit_mask, req, need)
    check(e, res, lab, req, need, counts)


# ---------------------------------------------------------------- h. across an update

@pytest.mark.parametrize("path", ["planes", "lds2", "swar", "i32"])
def test_knife_nodes_move_across_an_update(engines, path_cases, path):
    """After one run pe_update_nodes moves half the knife nodes from v to v - 1 and a quarter from v - 1 to v;
    pe_fit_mask_run, with no new upload, must see the new side of every value: ranks, planes and compressed
    residuals are rebuilt from the residuals, not kept."""
    bits, stat, extra, _, kind, W = PATHS[path]
    req, need, inv = path_cases[kind]
    e = engines(bits)
    res, lab = load(e, inv)
    counts = counted(e, stat, extra, e.fit_mask, req, need, W=W)
    first = check(e, res, lab, req, need, counts)
    rng = np.random.default_rng(5)
    at_v, below = np.flatnonzero(inv.knife_delta == 0), np.flatnonzero(inv.knife_delta == -1)
    at_v = at_v[inv.knife_dim[at_v] >= 0]
    down = rng.choice(at_v, len(at_v) // 2, replace=False)
    up = rng.choice(below, len(below) // 4, replace=False)
    for slots, step in ((down, -1), (up, 1)):
        res[inv.knife_dim[slots], slots] += step
    slots = np.concatenate([down, up])
    cap, used = FT.split_residual(res[:, slots])
    e.update_nodes(slots, np.zeros(len(slots), np.uint8), np.ascontiguousarray(cap.T), np.ascontiguousarray(used.T),
                   inv.labels[slots], inv.island[slots])
    np.testing.assert_array_equal(e.read_residuals(), res)
    counted(e, stat, extra, e.fit_mask_run, W=W)
    after = check(e, res, lab, req, need)
    assert (after != first).any()
