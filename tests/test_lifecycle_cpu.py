"""The float64 reference of the surfel lifecycle and of the activation pass (tests/lifecycle_util.py) on its own and against the
oracle (oracle/bso_lifecycle.c, bso_update_surfel_activation); no GPU.

  * the census: every branch the GPU tests are meant to decide is reached by a DECIDED case of the fixtures, and at most 2 % of the
    surfels, cells and candidate pixels of any run are left out as ambiguous;
  * reference against oracle, decision by decision: merge after every keyframe, creation (filtered and not), deletion + radius
    update, compaction, activation -- the same checks (lifecycle_util.check_*) the GPU tests put the kernels through;
  * every reference decision is live: each of lifecycle_util.MUTATIONS, switched on, makes one of those checks fail;
  * C, measured: the created position and d1 / d2 in np.float32 against float64, as |d| / (2^-24 A):
        position 3.28 (recorded 3.3)     d1 / d2 0.18 (recorded 0.2)
  * the integer compaction reference against a sequential loop on random masks.
"""
import numpy as np
import pytest

from badslam_amd import abi
from tests import lifecycle_util as L
from tests import surfel_terms_util as ST
from tests.lifecycle_util import OracleBackend

def test_constants_agree():
    assert (L.KF_ACTIVE, L.KF_COVISIBLE_ACTIVE, L.KF_INACTIVE) == (abi.KF_ACTIVE, abi.KF_COVISIBLE_ACTIVE, abi.KF_INACTIVE)
    assert L.INVALID_DEPTH_BIT == abi.BSLAM_INVALID_DEPTH_BIT and L.SURFEL_ACTIVE_FLAG == abi.BSLAM_SURFEL_ACTIVE_FLAG
    assert (L.TEX_FIXED_POINT_1_8, L.TEX_EXACT_FLOAT) == (abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT)
    assert L.INVALID_INDEX == abi.INVALID_INDEX


# ---- the census ---------------------------------------------------------------------------------------------------------
def merge_census(fixture, factor, census, shares):
    inp = fixture.inputs
    x, unknown = inp.surfels[L.ROW_X].copy(), np.zeros(fixture.N, bool)
    dead = L.is_deleted(inp.surfels[L.ROW_X])
    for k in range(len(inp.keyframes)):
        m = L.merge_step(inp, k, inp.surfels, x, factor, np.float64, unknown)
        s, sure = m.support, ~m.ambiguous
        counts = np.array([len(s.members.get(c, ())) for c in range(s.cells_w * s.cells_h)]).reshape(s.cells_h, s.cells_w)
        for name, part in (("cells", counts), ("right column", counts[:, -1]), ("bottom row", counts[-1])):
            for n in range(5):
                census[f"{name} with {'more than 3' if n == 4 else n} associated surfels"] += int((np.minimum(part, 4) == n).sum())
        other = m.rank == 3
        census["holder 1 merged by holder 0"] += int(((m.rank == 1) & m.close[0] & m.deleted & sure).sum())
        census["holder 2 merged by holder 0"] += int(((m.rank == 2) & m.close[0] & m.deleted & sure).sum())
        census["holder 2 merged by holder 1 alone, holder 1 surviving"] += int(((m.rank == 2) & ~m.close[0] & m.close[1] & m.deleted & sure).sum())
        census["holder 2 kept because holder 1 was merged first"] += int((m.kept_by_order & ~m.gone & sure).sum())
        for b in range(3):
            alone = m.close[b] & ~np.delete(m.close, b, 0).any(0)
            census[f"a non-holder merged by holder {b} only"] += int((other & alone & m.deleted & sure).sum())
        census["a non-holder kept"] += int((other & ~m.gone & sure).sum())
        census["a pre-existing NaN surfel as holder 0 of cell (0, 0)"] += int(s.holders[0, 0] != L.INVALID_INDEX and dead[s.holders[0, 0]] and not s.cell_ambiguous[0])
        census["a merge refused by the normal test alone"] += int((m.near_ok & ~m.normal_ok & sure).sum())
        census["a merge refused by the distance test alone"] += int((m.normal_ok & ~m.near_ok & sure).sum())
        shares.append(("merge", fixture.case, fixture.variant, factor, k, float(m.ambiguous.mean()), float(s.cell_ambiguous.mean())))
        x[m.deleted] = L.nan_x()
        unknown |= m.ambiguous


def creation_census(fixture, census, shares):
    inp = fixture.inputs
    w, h = inp.cameras[1][4:]
    for k, share, filtered, min_count, covis, mode in L.CREATION_RUNS:
        size = L.size_of(fixture, share)
        c = L.creation(inp, k, inp.surfels[:, :size], inp.surfels[L.ROW_X, :size], filtered, min_count, L.covis_list(fixture, k, list(covis)), L.MODES[mode], np.float64, with_columns=False)
        s = c.support
        depth = inp.keyframes[k]["depth"]
        ys, xs = c.candidates // w, c.candidates % w
        first = (ys % inp.cell == 0) & (xs % inp.cell == 0)
        cell_first_is_hole = (depth[ys - ys % inp.cell, xs - xs % inp.cell] & L.INVALID_DEPTH_BIT) != 0
        inner = (ys - ys % inp.cell >= 1) & (xs - xs % inp.cell >= 1)
        census["creation in a cell whose first pixels are holes"] += int((~first & cell_first_is_hole & inner & ~c.candidate_ambiguous).sum())
        partial = (xs // inp.cell == s.cells_w - 1) & (w % inp.cell != 0) | (ys // inp.cell == s.cells_h - 1) & (h % inp.cell != 0)
        census["creation in a partial cell"] += int((partial & ~c.candidate_ambiguous).sum())
        # free cells without a candidate although a border pixel of theirs has a measurement
        gy, gx = np.mgrid[0:h, 0:w]
        cell_id = (gy // inp.cell) * s.cells_w + gx // inp.cell
        border_valid = ((gx == 0) | (gy == 0) | (gx == w - 1) | (gy == h - 1)) & ((depth & L.INVALID_DEPTH_BIT) == 0)
        has_border_valid = np.zeros(s.cells_w * s.cells_h, bool)
        has_border_valid[cell_id[border_valid]] = True
        chosen = np.zeros(s.cells_w * s.cells_h, bool)
        chosen[cell_id.ravel()[c.candidates]] = True
        census["a free border cell where only border pixels are valid: nothing created"] += int((has_border_valid & ~chosen & ~c.occupied & ~c.cell_undecided).sum())
        if filtered:
            sure = ~c.kept_ambiguous & ~c.candidate_ambiguous
            low, limit = L.u16(min_count), L.u16(c.observations)
            census["filter: kept"] += int((c.kept & sure).sum())
            census["filter: kept with exactly min_observation_count observations"] += int((c.kept & sure & (limit == low) & (len(covis) > 0)).sum())
            census["filter: removed, one observation short"] += int((~c.kept & sure & (limit == low - 1)).sum())
            census["filter: kept with violations == observations"] += int((c.kept & sure & (c.violations == c.observations)).sum())
            census["filter: removed, one violation too many"] += int((~c.kept & sure & (limit >= low) & (c.violations == c.observations + 1)).sum())
        shares.append(("creation", fixture.case, fixture.variant, k, size, float((c.candidate_ambiguous | c.kept_ambiguous).mean()) if len(c.candidates) else 0.0,
                       float(c.cell_undecided.mean())))


def deletion_census(fixture, census, shares):
    inp = fixture.inputs
    for min_count in (1, 2, 3):
        d = L.deletion(inp, inp.surfels, inp.surfels[L.ROW_X], min_count, np.float64)
        sure = ~d.ambiguous
        census[f"deletion by obs < min at min_observation_count {min_count}"] += int((sure & d.deleted & (d.observations < min_count)).sum())
        census[f"deletion one observation short at min_observation_count {min_count}"] += int((sure & d.deleted & (d.observations == min_count - 1)).sum())
        census["deletion by viol > obs"] += int((sure & d.deleted & (d.observations >= min_count) & (d.violations > d.observations)).sum())
        census["viol == obs kept"] += int((sure & d.survives & (d.violations == d.observations) & (d.observations > 0)).sum())
        census["a survivor whose minimum radius is not the first associated keyframe's"] += int((sure & d.survives & (d.radius != d.radius_of_first)).sum())
        census["an already deleted surfel meets the deletion test again"] += int((sure & L.is_deleted(inp.surfels[L.ROW_X]) & ~d.survives).sum())
        shares.append(("deletion", fixture.case, fixture.variant, min_count, float(d.ambiguous.mean())))


def activation_census(fixture, census, shares):
    associated, ambiguous = L.ba_terms(fixture.inputs)
    before = fixture.inputs.active
    for name, mask in L.ACTIVITY_MASKS.items():
        new, undecided = L.activation(associated, ambiguous, mask, before)
        on = np.array(mask) == L.KF_ACTIVE
        was = (before & 1) != 0
        census["activation: an active surfel whose only associated keyframes are inactive"] += int((was & ~undecided & associated[:, ~on].any(1) & ~associated[:, on].any(1)).sum())
        census["activation: other bits of the byte, surfel stays inactive"] += int((~undecided & ((before & 0xFE) != 0) & ((new & 1) == 0)).sum())
        census["activation: other bits of the byte, surfel activated"] += int((~undecided & ((before & 0xFE) != 0) & ((new & 1) != 0)).sum())
        census["activation: an inactive surfel is activated"] += int((~was & ~undecided & ((new & 1) != 0)).sum())
        shares.append(("activation", fixture.case, fixture.variant, name, float(undecided.mean())))


def test_census(capsys):
    from collections import Counter
    census, shares = Counter(), []
    required = set()
    for case, variant in L.RUNS:
        fixture = L.lifecycle_fixture(case, variant)
        local = Counter()
        for factor in L.FACTORS:
            merge_census(fixture, factor, local, shares)
        creation_census(fixture, local, shares)
        deletion_census(fixture, local, shares)
        if variant == "cell4":
            activation_census(fixture, local, shares)
        census.update(local)
        required |= set(local)
        with capsys.disabled():
            print(f"\ncensus of {case} / {variant}:")
            for name in sorted(local):
                print(f"  {local[name]:6d}  {name}")
    missing = [name for name in sorted(required) if census[name] == 0]          # the partial cells' five counts among them
    assert not missing, missing
    worst = max(max(entry[5:] if entry[0] in ("merge", "creation") else entry[4:]) for entry in shares)
    with capsys.disabled():
        print(f"largest ambiguous share of any run: {worst:.4f}")
    over = [entry for entry in shares if max(entry[5:] if entry[0] in ("merge", "creation") else entry[4:]) > L.MAX_AMBIGUOUS_SHARE]
    assert not over, over


# ---- reference against oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", L.FACTORS)
@pytest.mark.parametrize("case,variant", L.RUNS)
def test_merge_matches_oracle(oracle, case, variant, factor):
    fixture = L.lifecycle_fixture(case, variant)
    assert not L.check_merge(fixture, factor, OracleBackend(L.scene_of(fixture)))


@pytest.mark.parametrize("case,variant", L.RUNS)
def test_creation_matches_oracle(oracle, case, variant):
    fixture = L.lifecycle_fixture(case, variant)
    failures, created = [], 0
    for k, share, filtered, min_count, covis, mode in L.CREATION_RUNS:
        f, c = L.check_creation(fixture, OracleBackend, k, L.size_of(fixture, share), filtered, min_count, list(covis), L.MODES[mode], (k, share, filtered, min_count, covis, mode))
        failures += f
        created += int(c.kept.sum())
    assert not failures, failures[:5]
    assert created > 100


def test_large_creation_matches_oracle(oracle):
    fixture = L.large_fixture()
    failures, c = L.check_creation(fixture, OracleBackend, 0, fixture.N, False, 2, [], abi.TEX_EXACT_FLOAT, "640x410")
    assert not failures, failures[:5]
    w = L.LARGE_SIZE[0]
    ys, xs = c.candidates // w, c.candidates % w
    # tile 255 of the pixel scan (pixels 261120 .. 262143: row 408 and the start of the border row) holds flags, so the count that the
    # call returns carries that tile's sum out of the first block of tile totals; no pixel from 262144 on can be a candidate (border)
    assert ((c.candidates >= 255 * 1024) & (c.candidates < 256 * 1024)).sum() >= 8 and not (c.candidates >= 256 * 1024).any()
    assert len(c.candidates) > 600 and len(set(zip((ys % L.LARGE_CELL).tolist(), (xs % L.LARGE_CELL).tolist()))) > 10      # the chosen pixel varies


@pytest.mark.parametrize("min_count", (1, 2, 3))
@pytest.mark.parametrize("case,variant", L.RUNS)
def test_deletion_matches_oracle(oracle, case, variant, min_count):
    fixture = L.lifecycle_fixture(case, variant)
    for keyframes, order in ((None, None), ([0, 1, 2], None), (None, np.arange(fixture.N)[::-1]), ([], None)):
        failures, d = L.check_deletion(fixture, OracleBackend, min_count, keyframes, order, label=(keyframes, order is not None))
        assert not failures, failures[:5]
        if keyframes == []:
            assert not d.survives.any()


def host_rows_backend(rows, active):
    from tests import bso
    cam = bso.make_camera(45.0, 44.0, 18.2, 11.7, 37, 23)
    scene = bso.HostScene(cam, cam, ST.RAW_TO_FLOAT_DEPTH, ST.BASELINE_FX, 4, rows.shape[1])
    scene.surfels.view(np.uint32)[:8] = rows
    scene.active[0] = active
    scene.surfels_size = rows.shape[1]
    return OracleBackend(scene)


@pytest.mark.parametrize("n", L.SIZES)
def test_compaction_matches_oracle(oracle, n):
    for pattern in L.PATTERNS:
        for with_active in (True, False):
            assert not L.check_compaction(host_rows_backend, n, pattern, with_active)


def test_compaction_against_a_sequential_loop():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(1, 90))
        rows, active, _ = L.compaction_case(n, "thirds", seed=trial)
        rows[L.ROW_X] = np.where(rng.random(n) < rng.random(), L.NAN_BITS, np.arange(n)).astype(np.uint32)
        count = int((rows[L.ROW_X] != L.NAN_BITS).sum())
        for with_active in (True, False):
            got = L.compaction(rows, active if with_active else None, n, count)
            want = L.compaction_brute_force(rows, active if with_active else None, n, count)
            assert np.array_equal(got[0], want[0]) and got[2] == want[2]
            assert (got[1] is None and want[1] is None) or np.array_equal(got[1], want[1])
            # what is left below the new size is exactly the valid surfels, each once
            assert sorted(got[0][1, :count].tolist()) == sorted(rows[1, rows[L.ROW_X] != L.NAN_BITS].tolist())


@pytest.mark.parametrize("mask", sorted(L.ACTIVITY_MASKS))
@pytest.mark.parametrize("case", sorted(ST.CASES))
def test_activation_matches_oracle(oracle, case, mask):
    fixture = L.lifecycle_fixture(case)
    associated, ambiguous = L.with_nan_surfels(fixture.inputs, fixture.inputs.keyframes, *L.ba_terms(fixture.inputs))
    failures, _, _ = L.check_activation(OracleBackend(L.activity_scene(fixture, L.ACTIVITY_MASKS[mask])), associated, ambiguous, L.ACTIVITY_MASKS[mask])
    assert not failures, failures


@pytest.mark.parametrize("K", (63, 64, 65))
def test_activation_of_a_long_stack_matches_oracle(oracle, K):
    fixture = L.lifecycle_fixture("same_camera")
    kfs = fixture.inputs.keyframes
    associated, ambiguous = L.with_nan_surfels(fixture.inputs, [kfs[5]] * (K - 1) + [kfs[0]], *L.stack_terms(fixture, K))
    failures, want, _ = L.check_activation(OracleBackend(L.stack_scene(fixture, K)), associated, ambiguous, [L.KF_ACTIVE] * K)
    assert not failures, failures
    assert (want & 1).sum() > 300


# ---- every reference decision is live --------------------------------------------------------------------------------------
def caught_by(mutation):
    """the failures of the check that is meant to notice the mutation"""
    fixture = L.lifecycle_fixture("same_camera")
    if mutation in ("holders_largest", "skip_holder_1_vs_2"):
        return [f for factor in L.FACTORS for f in L.check_merge(fixture, factor, OracleBackend(L.scene_of(fixture)))]
    if mutation in ("viol_ge_obs", "radius_first_keyframe"):
        return L.check_deletion(fixture, OracleBackend, 1)[0]
    if mutation == "border_0":
        return L.check_creation(fixture, OracleBackend, 0, 0, False, 2, [], abi.TEX_EXACT_FLOAT)[0]
    if mutation == "cells_floor":
        return L.check_creation(fixture, OracleBackend, 1, L.size_of(fixture, 0.15), False, 2, [], abi.TEX_EXACT_FLOAT)[0] + \
            L.check_merge(fixture, 0.8, OracleBackend(L.scene_of(fixture)))
    if mutation == "scan_carry":
        return L.check_compaction(host_rows_backend, 264200, "late", True) + L.check_compaction(host_rows_backend, 264200, "early", False)
    raise KeyError(mutation)


@pytest.mark.parametrize("mutation", L.MUTATIONS)
def test_mutation_is_caught(oracle, monkeypatch, mutation):
    assert not caught_by(mutation), "the check fails on the unmutated reference"
    monkeypatch.setattr(L, "MUTATION", mutation)
    assert caught_by(mutation), f"no decided case of the fixture tells the reference from its mutation {mutation}"


def test_measured_c(capsys):
    measured = L.measure_c()
    with capsys.disabled():
        print("\nmeasured C:", {kind: round(value, 3) for kind, value in measured.items()})
    for kind, value in measured.items():
        assert value <= L.C_MEASURED[kind], (kind, value)
        assert value >= 0.3 * L.C_MEASURED[kind], (kind, value, "the recorded C is far above what is measured")
