"""-m gpu: pose_accumulate_kernel in both designs (csrc/pose_kernels.hpp) and the geometry iteration (geometry_normals_kernel,
geometry_position_kernel, geometry_position_chunk_kernel, geometry_desc_chunk_kernel, csrc/geometry_kernels.hpp) against a float64
reference of the same operation, one (surfel, keyframe) pair and one surfel at a time.

The public entry points are the probe: a surfel buffer that holds ONE surfel returns, from bslam_accumulate_pose_coeffs_batched, the
K pair rows of that surfel (adding zeros is exact), and the geometry entry points return every surfel's own step.  The reference
is tests/surfel_terms_util.py in float64 on its hard fixture (tests/test_surfel_terms_cpu.py has the census and checks the
reference on its own and against the oracle).

Tolerance of a value: |got - value64| <= 4 * C * 2^-24 * A (+ the fixed-point texture mode's widening), A being the value
evaluated with absolute values and C what the same formulas in plain np.float32 reach on the fixture, measured on the CPU and
recomputed by test_surfel_terms_cpu.py::test_measured_c:

    C[depth] = 6.73 (recorded 6.8)   C[desc] = 1.30 (1.4)   C[normals] = 2.18 (2.2)   C[position] = 1.38 (1.4)   C[joint] = 2.49 (2.5)

(a row with both residual kinds: each kind's share of A with its own C).  The factor 4 is the project's KERNEL_FACTOR (fused
multiply-adds, the 1-ulp v_rcp_f32 of rdiv / rrcp, another association).  A stored position is an fp32 number next to the old
one, so a step is known from (new - old) . n only to the rounding of the stored components; that rounding (2^-24 per component,
twice) is added to the step's tolerance and stated in surfel_terms_util.check_geometry.

n_add, the longest chain of fp32 additions between a pair's term and the returned row:
  geometry-only design (4 surfels per lane, 8 columns per round)                                                          49
    accumulate_h_b (csrc/pose_kernels.hpp:93, :99): one fused add per surfel of the lane                                    4
    wave_column_sums_lds (csrc/device_math.hpp:1241-1244: 3 in stage 1; :1258: 2 in stage 2; :1259: one DPP add)           6
    RowStash::flush (csrc/device_math.hpp:1301): ((w0 + w1) + w2) + w3                                                      3
    column_share_of_rows (csrc/pose_kernels.hpp:533: one add per pass of 256 rows, one pass here; :536: 3)                 4
    pose_reduce_rows_kernel (csrc/pose_kernels.hpp:577): the 32 partial sums of a column, in sequence                     32
  photometric design (8 surfels per lane, 4 columns per round, one wave per row)                                          66
    accumulate_h_b and accumulate_h_b_desc_pair (csrc/device_math.hpp:902-918: up to two adds per entry): 3 per pair, x 8  24
    wave_column_sums_lds (:1241: 2; :1258: 2; :1259-1260: two DPP adds)                                                     6
    column_share_of_rows and pose_reduce_rows_kernel as above                                                              36

Time, measured on MI355X (the kernels are the parent commit's: this module changes none): a one-surfel batched call -- a
one-column device copy, the keyframe table, the accumulation, the row sum and a read-back -- takes about 40 us, a one-surfel
per-keyframe call with the cost the same.  A case of the every-pair test is 1317 calls, 0.05 to 0.13 s, with its comparison
under 0.3 s; a case of the cost test is 6 x 300 calls, 0.07 s; a case of the full-set test 7 calls; a geometry case one call of
0.1 to 0.3 ms.  The whole module takes 5.4 s, 1.7 s of it the first context.  No case comes near a second, so the
parametrisation is (case, variant, mode) and no pair of the kCost = false path is left out.
"""
import ctypes as C
import time

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import surfel_terms_util as U
from tests.gpu_util import Hip, stream_ptr

pytestmark = pytest.mark.gpu
P = C.POINTER
MODES = {"fixed": abi.TEX_FIXED_POINT_1_8, "exact": abi.TEX_EXACT_FLOAT}
N_ADD = {False: 4 + 6 + 3 + 4 + 32, True: 24 + 6 + 4 + 32}          # by use_desc
# (use_depth, use_desc, mode): the depth rows do not read the texture
PAIR_RUNS = [(1, 0, "exact"), (0, 1, "fixed"), (0, 1, "exact"), (1, 1, "fixed"), (1, 1, "exact")]
COST_SUBSET = 300


def _fp(a):
    return a.ctypes.data_as(P(C.c_float))


class Bench:
    """The library, one context, the device scene of every case and a one-surfel probe buffer."""

    def __init__(self):
        import torch
        self.torch, self.L, self.ctx = torch, badslam_amd.lib(), badslam_amd.Context(0)
        self.scenes, self.cache = {}, {}
        self.probe = torch.zeros((abi.SURFEL_ATTRIBUTE_COUNT, 64), dtype=torch.float32, device="cuda:0")

    def close(self):
        self.ctx.close()

    def scene(self, case):
        if case not in self.scenes:
            host = U.scene_copy(case, 1, 1, abi.TEX_EXACT_FLOAT)
            self.scenes[case] = host.to_device()
        return self.scenes[case]

    def batched(self, case, use_depth, use_desc, surfel_buf, size):
        """-> a function returning uint32 [K, 32] rows of one bslam_accumulate_pose_coeffs_batched call"""
        dev = self.scene(case)
        dp, kfs, K = dev.depth_params(), dev.keyframe_views(), U.N_KEYFRAMES
        Hb, counts = np.zeros((K, 27), np.float32), np.zeros(K, np.uint32)
        args = (self.ctx.handle, stream_ptr(), use_depth, use_desc, C.byref(dev.host.color_camera), C.byref(dev.host.depth_camera), C.byref(dp), K, kfs,
                size, C.byref(surfel_buf), _fp(Hb), counts.ctypes.data_as(P(C.c_uint32)))

        def call(out):
            badslam_amd.check(self.L.bslam_accumulate_pose_coeffs_batched(*args))
            out[:, :27] = Hb.view(np.uint32)
            out[:, U.COL_COUNT] = counts
            return out
        call.keep = (dp, kfs, surfel_buf)
        return call

    def single(self, case, use_depth, use_desc, k, surfel_buf, size):
        """-> a function returning the uint32 [32] row of one bslam_accumulate_pose_estimation_coeffs call (keyframe k, with the cost)"""
        dev = self.scene(case)
        dp, v = dev.depth_params(), dev.keyframe_view(k)
        H, b, count, cost = np.zeros(21, np.float32), np.zeros(6, np.float32), C.c_uint32(), C.c_float()
        args = (self.ctx.handle, stream_ptr(), use_depth, use_desc, C.byref(dev.host.color_camera), C.byref(dev.host.depth_camera), C.byref(dp),
                C.byref(v.depth), C.byref(v.normals), C.byref(v.color), C.byref(v.frame_T_global), size, C.byref(surfel_buf), 1,
                C.byref(count), C.byref(cost), _fp(H), _fp(b))

        def call(out):
            badslam_amd.check(self.L.bslam_accumulate_pose_estimation_coeffs(*args))
            out[:21], out[21:27] = H.view(np.uint32), b.view(np.uint32)
            out[U.COL_COST] = np.array([cost.value], np.float32).view(np.uint32)[0]
            out[U.COL_COUNT] = count.value
            return out
        call.keep = (dp, v, surfel_buf)
        return call

    def pair_rows(self, case, use_depth, use_desc, mode):
        """uint32 [N, K, 32]: the K rows of every surfel alone in the buffer (kCost = false, the kernel bundle adjustment runs)"""
        key = ("pair", case, use_depth, use_desc, mode)
        if key not in self.cache:
            self.ctx.set_texture_mode(MODES[mode])
            dev, probe = self.scene(case), self.probe
            call = self.batched(case, use_depth, use_desc, dev.tbuf(probe), 1)
            rows = np.zeros((U.N_SURFELS, U.N_KEYFRAMES, U.ROW), np.uint32)
            start = time.perf_counter()
            for i in range(U.N_SURFELS):
                probe[:8, 0:1] = dev.surfels[:8, i:i + 1]
                call(rows[i])
            print(f"{case} {U.variant_name(use_depth, use_desc)} {mode}: {U.N_SURFELS} one-surfel batched calls in {time.perf_counter() - start:.2f} s")
            self.cache[key] = rows
        return self.cache[key]

    def cost_rows(self, case, use_depth, use_desc, mode, subset):
        """uint32 [len(subset), K, 32]: the same through the per-keyframe entry point with the cost column (kCost = true)"""
        key = ("cost", case, use_depth, use_desc, mode)
        if key not in self.cache:
            self.ctx.set_texture_mode(MODES[mode])
            dev, probe = self.scene(case), self.probe
            calls = [self.single(case, use_depth, use_desc, k, dev.tbuf(probe), 1) for k in range(U.N_KEYFRAMES)]
            rows = np.zeros((len(subset), U.N_KEYFRAMES, U.ROW), np.uint32)
            start = time.perf_counter()
            for j, i in enumerate(subset):
                probe[:8, 0:1] = dev.surfels[:8, i:i + 1]
                for k, call in enumerate(calls):
                    call(rows[j, k])
            print(f"{case} {U.variant_name(use_depth, use_desc)} {mode}: {len(subset) * U.N_KEYFRAMES} one-surfel cost calls in {time.perf_counter() - start:.2f} s")
            self.cache[key] = rows
        return self.cache[key]

    def full_rows(self, case, use_depth, use_desc, mode):
        """uint32 [2, K, 32]: all N surfels through the batched entry point and through the per-keyframe one"""
        self.ctx.set_texture_mode(MODES[mode])
        dev = self.scene(case)
        rows = np.zeros((2, U.N_KEYFRAMES, U.ROW), np.uint32)
        self.batched(case, use_depth, use_desc, dev.surfel_buf(), U.N_SURFELS)(rows[0])
        for k in range(U.N_KEYFRAMES):
            self.single(case, use_depth, use_desc, k, dev.surfel_buf(), U.N_SURFELS)(rows[1, k])
        return rows


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def decode(rows):
    """uint32 rows -> float64 values, the count column as the integer it is"""
    out = rows.view(np.float32).astype(np.float64)
    out[..., U.COL_COUNT] = rows[..., U.COL_COUNT]
    return out


def compare_rows(terms, rows, columns, label):
    """rows uint32 [n, K, 32] of the surfels terms was cut to: count, zero rows, values -> failures"""
    got = decode(rows)
    tolerance = U.pair_tolerance(terms)
    failures = []
    if not np.isfinite(got).all():
        return [(label, "not finite")]
    decided = ~terms.ambiguous
    has_row = terms.row[..., U.COL_COUNT] > 0
    wrong_count = decided & (got[..., U.COL_COUNT] != terms.row[..., U.COL_COUNT])
    nonzero = decided & ~has_row & (rows != 0).any(-1)
    compare = decided & has_row & ~wrong_count
    excess = (np.abs(got - terms.row) - tolerance)[..., columns]
    outside = compare[..., None] & (excess > 0)
    A = terms.A[..., columns]
    ratio = np.where(compare[..., None] & (A > 0), np.maximum(np.abs(got - terms.row)[..., columns] - terms.widen[..., columns], 0) / np.where(A > 0, U.EPS32 * A, 1), 0)
    print(f"{label}: rows {int(has_row.sum())} ambiguous {int(terms.ambiguous.sum())} largest |got - row64| / (2^-24 A) = {ratio.max():.3f}")
    for what, mask in (("count", wrong_count), ("row of a rejected pair is not zero", nonzero), ("value", outside.any(-1))):
        if mask.any():
            i, k = [int(v[0]) for v in np.nonzero(mask)]
            failures.append((label, what, int(mask.sum()), (i, k), U.STAGES[terms.stage[i, k]], [columns[c] for c in np.nonzero(outside[i, k])[0]], float(ratio[i, k].max())))
    return failures


H_AND_B = list(range(27)) + [U.COL_COUNT]
WITH_COST = list(range(28)) + [U.COL_COUNT]


@pytest.mark.parametrize("use_depth,use_desc,mode", PAIR_RUNS)
@pytest.mark.parametrize("case", list(U.CASES))
def test_every_pair_has_the_reference_row(bench, case, use_depth, use_desc, mode):
    """Every surfel alone through bslam_accumulate_pose_coeffs_batched: its K rows are its K pair rows.  The count is the reference's off
    the ambiguous pairs, a rejected pair's row is all zero bit for bit, every column lies within 4 C 2^-24 A (+ widening)."""
    terms = U.hard_terms(case, use_depth, use_desc, MODES[mode])
    rows = bench.pair_rows(case, use_depth, use_desc, mode)
    assert (rows[..., U.COL_COST] == 0).all()
    failures = compare_rows(terms, rows, H_AND_B, f"{case} {U.variant_name(use_depth, use_desc)} {mode}")
    assert not failures, failures


def cost_subset(case):
    """About 300 surfels: every surfel of a pair stage or robust half with fewer than 32 pairs, then every fourth surfel"""
    terms = U.hard_terms(case, 1, 1, MODES["exact"])
    chosen = set()
    classes = [terms.stage == s for s in range(len(U.STAGES))]
    raw = np.abs(terms.terms["depth"]["r"].v)
    classes += [terms.associated & (raw >= 10)] + [terms.has_desc & ((np.abs(terms.terms[n]["r"].v) < 10) == inside) for n in ("desc1", "desc2") for inside in (True, False)]
    classes += [terms.has_desc & terms.border]
    for members in classes:
        if 0 < members.sum() < 32:
            chosen.update(np.nonzero(members.any(1))[0].tolist())
    for i in range(0, U.N_SURFELS, 4):
        if len(chosen) >= COST_SUBSET:
            break
        chosen.add(i)
    return np.array(sorted(chosen))


class Cut:
    """the reference's arrays of a subset of the surfels"""

    def __init__(self, terms, subset):
        for name in ("row", "A", "A_depth", "A_desc", "widen", "ambiguous", "stage"):
            setattr(self, name, getattr(terms, name)[subset])


@pytest.mark.parametrize("use_depth,use_desc,mode", PAIR_RUNS)
@pytest.mark.parametrize("case", list(U.CASES))
def test_the_cost_column(bench, case, use_depth, use_desc, mode):
    """The same through bslam_accumulate_pose_estimation_coeffs (kCost = true, one keyframe per call) on a fixed subset: H, b, the
    count and the cost (quirk Q1: the first descriptor residual only)."""
    subset = cost_subset(case)
    assert 250 <= len(subset) <= 400
    terms = Cut(U.hard_terms(case, use_depth, use_desc, MODES[mode]), subset)
    rows = bench.cost_rows(case, use_depth, use_desc, mode, subset)
    failures = compare_rows(terms, rows, WITH_COST, f"{case} {U.variant_name(use_depth, use_desc)} {mode} cost")
    assert (decode(rows)[..., U.COL_COST] > 0).sum() > 100
    assert not failures, failures


@pytest.mark.parametrize("use_depth,use_desc,mode", PAIR_RUNS)
@pytest.mark.parametrize("case", list(U.CASES))
def test_full_set_row_is_the_sum_of_its_pairs(bench, case, use_depth, use_desc, mode):
    """Lanes, slots, tails: the row of each keyframe over all N surfels (both entry points) against the float64 sum of the kernel's own
    one-surfel rows -- within (n_add + 1) 2^-24 sum |own rows|, equal counts -- and against the reference's sum with the summed
    tolerances (an ambiguous pair enters that sum as the kernel's own row)."""
    terms = U.hard_terms(case, use_depth, use_desc, MODES[mode])
    own = decode(bench.pair_rows(case, use_depth, use_desc, mode))
    full = decode(bench.full_rows(case, use_depth, use_desc, mode))
    n_add = N_ADD[bool(use_desc)]
    values = list(range(27))
    own_sum, bound = own.sum(0), (n_add + 1) * U.EPS32 * np.abs(own).sum(0)
    ambiguous = terms.ambiguous[..., None]
    want = np.where(ambiguous, own, terms.row).sum(0)
    allowed = np.where(ambiguous, 0, U.pair_tolerance(terms)).sum(0) + (n_add + 1) * U.EPS32 * np.abs(np.where(ambiguous, own, terms.row)).sum(0)
    failures = []
    for e, entry in enumerate(("batched", "per keyframe")):
        for k in range(U.N_KEYFRAMES):
            if full[e, k, U.COL_COUNT] != own_sum[k, U.COL_COUNT]:
                failures.append((entry, k, "count", full[e, k, U.COL_COUNT], own_sum[k, U.COL_COUNT]))
            worst = np.where(bound[k, values] > 0, np.abs(full[e, k] - own_sum[k])[values] / np.where(bound[k, values] > 0, bound[k, values], 1), 0).max()
            print(f"{case} {U.variant_name(use_depth, use_desc)} {mode} {entry} keyframe {k}: count {int(full[e, k, U.COL_COUNT])} |full - own| / bound = {worst:.3f}")
            if (np.abs(full[e, k] - own_sum[k])[values] > bound[k, values]).any():
                failures.append((entry, k, "own rows", np.nonzero(np.abs(full[e, k] - own_sum[k])[values] > bound[k, values])[0].tolist()))
            if (np.abs(full[e, k] - want[k])[values] > allowed[k, values]).any() or full[e, k, U.COL_COUNT] != want[k, U.COL_COUNT]:
                failures.append((entry, k, "reference", np.nonzero(np.abs(full[e, k] - want[k])[values] > allowed[k, values])[0].tolist()))
        cost, cost_allowed = terms.row[..., U.COL_COST].sum(0), U.pair_tolerance(terms)[..., U.COL_COST].sum(0) + (n_add + 1) * U.EPS32 * np.abs(terms.row[..., U.COL_COST]).sum(0)
        if e == 1 and not terms.ambiguous.any() and (np.abs(full[1, :, U.COL_COST] - cost) > cost_allowed).any():
            failures.append((entry, "cost", full[1, :, U.COL_COST].tolist(), cost.tolist()))
    assert full[0, :U.N_KEYFRAMES - 1, U.COL_COUNT].min() > 100 and full[0, U.N_KEYFRAMES - 1, U.COL_COUNT] == 0
    assert not failures, failures


# what runs, (use_depth, use_desc), the keyframe chunk
GEOMETRY_RUNS = {"normals": (1, 0, -1), "geometry_only": (1, 0, -1), "geometry_only_chunked": (1, 0, 2), "photometric": (1, 1, -1),
                 "photometric_chunked": (1, 1, 2), "photometric_without_depth": (0, 1, -1)}


# the runs that read no texture are the same in both modes
GEOMETRY_CASES = [(run, mode) for run, (_, use_desc, _) in GEOMETRY_RUNS.items() for mode in (MODES if use_desc else ("exact",))]


@pytest.mark.parametrize("run,mode", GEOMETRY_CASES)
@pytest.mark.parametrize("case", list(U.CASES))
def test_geometry_iteration_per_surfel(bench, case, run, mode):
    """bslam_update_surfel_normals and bslam_optimize_geometry_iteration on all N surfels: the packed normals equal the reference's code off
    the ambiguous surfels, the STEP -- (new - old) . n and d_new - d_old -- lies within 4 C[step] 2^-24 A_step, the move across the
    normal within a few roundings, a surfel behind a closed guard keeps its eight rows bit for bit, clamped descriptors are +-180."""
    use_depth, use_desc, chunk = GEOMETRY_RUNS[run]
    g = U.hard_geometry(case, use_depth, use_desc, MODES[mode])
    host = U.scene_copy(case, use_depth, use_desc, MODES[mode])
    before = np.array(host.surfels)
    dev = host.to_device()
    hip = Hip(dev, ctx=bench.ctx)
    badslam_amd.check(bench.L.bslam_set_geometry_keyframe_chunk(bench.ctx.handle, chunk))
    start = time.perf_counter()
    try:
        if run == "normals":
            hip.update_normals()
        else:
            hip.optimize_geometry_iteration()
    finally:
        badslam_amd.check(bench.L.bslam_set_geometry_keyframe_chunk(bench.ctx.handle, -1))
    print(f"{case} {run} {mode}: {time.perf_counter() - start:.4f} s")
    after, active = dev.surfels_np(), dev.active_np()
    assert np.array_equal(active, host.active), "the active flags are read only"
    assert np.array_equal(after[8:].view(np.uint32), before[8:].view(np.uint32)) and np.array_equal(after[:, U.N_SURFELS:].view(np.uint32), before[:, U.N_SURFELS:].view(np.uint32))
    if run == "normals":
        bits = lambda rows: np.ascontiguousarray(rows[:8, :U.N_SURFELS]).view(np.uint32)
        a, b = bits(after), bits(before)
        decided = ~g.normal_ambiguous
        assert np.array_equal(a[U.ROW_NORMAL][decided], g.code[decided])
        others = [r for r in range(8) if r != U.ROW_NORMAL]
        assert np.array_equal(a[others], b[others])
        assert (a[U.ROW_NORMAL] != b[U.ROW_NORMAL]).sum() > 500
        return
    failures = U.check_geometry(g, before, after, bool(use_desc), (case, run, mode))
    assert not failures, failures
