"""The parity harness itself (tests/kernel_parity.py), without a GPU: a harness that compares nothing
passes everything, so each comparison path is shown to fail on the smallest difference it is there to
find.  The device scene is a fake that answers from the oracle on the Cornell box, with one edit where a
test asks for it: 256 rays of rays(256, 1), traced at depth 2."""
import os

import numpy as np
import pytest

import kernel_parity as KP
from kernel_parity import T_MAX, T_MIN

F = np.float32
DEPTH, SEED, V = 2, 17, 1
ROW = 17


class FakeScene:
    """What check_trace and hits_wrong use of a DeviceScene, answered by the oracle; `edit` changes an
    answer in place before it is returned, `report` is the variant kernel_info() names instead of the
    forced one."""

    def __init__(self, flat, osc, edit=None, report=None):
        self.flat, self.osc, self.edit, self.report = flat, osc, edit, report
        self.traced = self.fault_checks = 0

    def kernel_info(self, n_items=None, flags=0):
        return dict(variant=self.report or (flags >> 8) & 0xFF, lds_scene=True, bvh_arity=8, stack=15, shade_fast=True)

    def trace_rays(self, o, d, depth, seed=0, flags=0):
        self.traced += 1
        L = self.osc.trace_rays(o, d, depth, seed=seed)
        if self.edit:
            self.edit(L)
        return L

    def closest_hits(self, o, d, tmin, tmax, any_hit=False, quantized=False):
        hit, t, tri, _ = self.osc.closest(o, d, tmin, tmax)
        ids = KP.hit_ids(hit, tri)
        if self.edit:
            self.edit(ids, t)
        return ids, t

    def check_faults(self):
        self.fault_checks += 1


@pytest.fixture(scope="module")
def case(cornell, oracle_scene):
    o, d = KP.rays(256, 1)
    ref = KP.OracleRefs().trace("cornell", oracle_scene, o, d, DEPTH, SEED, False)
    assert ref.shape == (256, 3) and np.isfinite(ref).all() and ref.mean() > 0
    return cornell[2], oracle_scene, o, d, ref


def _trace(ds, case, **kw):
    _, _, o, d, ref = case
    KP.check_trace(ds, ref, o, d, DEPTH, SEED, V, label="harness", lds_scene=True, width=8,
                   expect={"shade_fast": True}, **kw)


# ------------------------------------------------------------------ check_trace
def test_the_oracles_own_answer_passes(case):
    flat, osc, o, d, _ = case
    ds = FakeScene(flat, osc)
    _trace(ds, case)
    assert ds.traced == 1 and ds.fault_checks == 1
    assert KP.hits_wrong(ds, osc, o, d, T_MIN, T_MAX, False, any_hit=False)[:2] == (0, [])
    n, first, ohit = KP.hits_wrong(ds, osc, o, d, T_MIN, KP.random_bounds(osc, o, d, 3), False, any_hit=True)
    assert (n, first) == (0, []) and 0.2 < ohit.mean() < 0.8


def test_one_flipped_mantissa_bit_fails_the_trace(case):
    flat, osc, _, _, ref = case

    def flip(L):
        L.view(np.uint32)[ROW, 1] ^= 1
    with pytest.raises(AssertionError) as e:
        _trace(FakeScene(flat, osc, edit=flip), case)
    label, v, count, ties, first = e.value.args[0]
    assert (label, v, count, ties) == ("harness", V, 1, None)
    assert len(first) == 1 and first[0][0] == ROW and np.array_equal(first[0][4], ref[ROW])
    with pytest.raises(AssertionError) as e:
        _trace(FakeScene(flat, osc, edit=flip), case, ties=np.arange(256) == ROW)
    assert e.value.args[0][3] == "1 of the differing rays are tie rays"


def test_another_variant_fails_before_the_trace(case):
    flat, osc = case[:2]
    ds = FakeScene(flat, osc, report=V + 1)
    with pytest.raises(AssertionError) as e:
        _trace(ds, case)
    assert e.value.args[0][:2] == ("harness", V) and ds.traced == 0


@pytest.mark.parametrize("kw", [dict(lds_scene=False), dict(width=4), dict(expect={"shade_fast": False})])
def test_another_kernel_fails_before_the_trace(case, kw):
    flat, osc, o, d, ref = case
    ds = FakeScene(flat, osc)
    with pytest.raises(AssertionError):
        KP.check_trace(ds, ref, o, d, DEPTH, SEED, V, label="harness", **kw)
    assert ds.traced == 0


def test_the_reference_has_to_be_what_the_case_is_for(case):
    flat, osc, o, d, ref = case
    ds = FakeScene(flat, osc)
    with pytest.raises(AssertionError):                     # a finite reference where an overflow is promised
        KP.check_trace(ds, ref, o, d, DEPTH, SEED, V, label="harness", finite=False)
    bad = ref.copy()
    bad[ROW, 0] = np.inf
    with pytest.raises(AssertionError):                     # and the other way round
        KP.check_trace(ds, bad, o, d, DEPTH, SEED, V, label="harness")
    with pytest.raises(AssertionError):                     # a black reference
        KP.check_trace(ds, np.zeros_like(ref), o, d, DEPTH, SEED, V, label="harness")
    assert ds.traced == 0


# ------------------------------------------------------------------ wrong_rows
def test_nan_payloads():
    a = np.array([[1, 2, 3], [4, np.nan, 6], [7, 8, 9]], F)
    b = a.copy()
    assert KP.wrong_rows(a, b).size == 0                    # the same payload: equal bits
    b.view(np.uint32)[1, 1] ^= 1
    assert np.isnan(b[1, 1])
    assert KP.wrong_rows(a, b, nan_aware=True).size == 0
    assert KP.wrong_rows(a, b, nan_aware=False).tolist() == [1]
    b[2, 0] = np.nextafter(b[2, 0], F(0))
    assert KP.wrong_rows(a, b, nan_aware=True).tolist() == [2]


# ------------------------------------------------------------------ hits_wrong
def _hit_row(case):
    _, osc, o, d, _ = case
    hit = osc.closest(o, d, T_MIN, T_MAX)[0] != 0
    assert hit[ROW]
    return ROW


def test_one_changed_id_is_one_offender(case):
    flat, osc, o, d, _ = case
    row = _hit_row(case)

    def edit(ids, t):
        ids[row] += 1
    n, first, _ = KP.hits_wrong(FakeScene(flat, osc, edit), osc, o, d, T_MIN, T_MAX, False, any_hit=False)
    assert n == 1 and first[0][0] == row and first[0][3] == first[0][4] + 1


def test_one_t_an_ulp_away_is_one_offender(case):
    flat, osc, o, d, _ = case
    row = _hit_row(case)

    def edit(ids, t):
        t[row] = np.nextafter(t[row], F(np.inf))
    n, first, _ = KP.hits_wrong(FakeScene(flat, osc, edit), osc, o, d, T_MIN, T_MAX, True, any_hit=False)
    assert n == 1 and first[0][0] == row and first[0][5] == np.nextafter(first[0][6], F(np.inf))


def test_a_hit_reported_as_a_miss_is_one_offender(case):
    flat, osc, o, d, _ = case
    tmax = KP.random_bounds(osc, o, d, 3)
    row = int(np.nonzero(osc.closest(o, d, T_MIN, tmax)[0])[0][0])

    def edit(ids, t):
        ids[row] = -1
    n, first, ohit = KP.hits_wrong(FakeScene(flat, osc, edit), osc, o, d, T_MIN, tmax, False, any_hit=True)
    assert n == 1 and first[0][0] == row and first[0][3] == tmax[row] and first[0][4] == -1 and ohit[row]
    # the oracle's answer handed in is used as it is
    n, _, _ = KP.hits_wrong(FakeScene(flat, osc, edit), osc, o, d, T_MIN, tmax, False, any_hit=True, want=ohit)
    assert n == 1


# ------------------------------------------------------------------ env_knobs
def test_env_knobs_restores(monkeypatch):
    monkeypatch.setenv("PRT_HARNESS_SET", "old")
    monkeypatch.delenv("PRT_HARNESS_UNSET", raising=False)
    with KP.env_knobs(PRT_HARNESS_SET=3, PRT_HARNESS_UNSET="x"):
        assert os.environ["PRT_HARNESS_SET"] == "3" and os.environ["PRT_HARNESS_UNSET"] == "x"
    assert os.environ["PRT_HARNESS_SET"] == "old" and "PRT_HARNESS_UNSET" not in os.environ
    with KP.env_knobs(PRT_HARNESS_SET=None):
        assert "PRT_HARNESS_SET" not in os.environ
    assert os.environ["PRT_HARNESS_SET"] == "old"
    with pytest.raises(KeyError):
        with KP.env_knobs(PRT_HARNESS_SET=4, PRT_HARNESS_UNSET=5):
            raise KeyError("the body fails")
    assert os.environ["PRT_HARNESS_SET"] == "old" and "PRT_HARNESS_UNSET" not in os.environ


# ------------------------------------------------------------------ the caches
class CountingOracle:
    def __init__(self):
        self.calls = []

    def trace_rays(self, o, d, depth, seed=0, nthreads=0):
        self.calls.append(("trace", depth, seed, nthreads))
        return np.ones((2, 3), F)

    def render_tiles(self, cam, W, H, tw, th, ids, spp, depth, seed=0, nthreads=0, counters=False):
        self.calls.append(("render", spp, depth, seed, counters))
        return np.ones((4, 3), F), np.array([0, 0, 5, 6])


def test_oracle_refs_compute_a_key_once():
    refs, osc = KP.OracleRefs(), CountingOracle()
    a = refs.trace(("case", 0), osc, None, None, 4, 17, False)
    assert refs.trace(("case", 0), osc, None, None, 4, 17, False) is a and len(osc.calls) == 1
    refs.trace(("case", 0), osc, None, None, 4, 17, True, nthreads=3)        # the estimator is part of the key
    refs.trace(("case", 1), osc, None, None, 4, 17, False)
    assert osc.calls == [("trace", 4, 17, 0), ("trace", 4, 17, 3), ("trace", 4, 17, 0)]
    r = refs.render_tiles("frame", osc, None, 8, 8, 8, None, 2, 4, 9)
    assert refs.render_tiles("frame", osc, None, 8, 8, 8, None, 2, 4, 9) is r and r[1] == (5, 6)
    assert osc.calls[3:] == [("render", 2, 4, 9, True)]
    assert KP.OracleRefs().trace(("case", 0), osc, None, None, 4, 17, False) is not a    # an instance per module


class StubScene:
    def __init__(self):
        self.knob, self.closed = os.environ.get("PRT_HARNESS_KNOB"), 0

    def close(self):
        self.closed += 1


def test_scene_cache_makes_each_scene_once_and_closes_it_once(monkeypatch):
    monkeypatch.delenv("PRT_HARNESS_KNOB", raising=False)
    gen = KP.scene_cache()
    make = next(gen)
    a = make("a", StubScene)
    a4 = make("a", StubScene, PRT_HARNESS_KNOB=4)
    b = make("b", StubScene, PRT_HARNESS_KNOB=None)
    assert make("a", StubScene) is a and make("a", StubScene, PRT_HARNESS_KNOB=4) is a4
    assert len({id(s) for s in (a, a4, b)}) == 3
    assert (a.knob, a4.knob, b.knob) == (None, "4", None) and "PRT_HARNESS_KNOB" not in os.environ
    assert (a.closed, a4.closed, b.closed) == (0, 0, 0)
    with pytest.raises(StopIteration):
        next(gen)
    assert (a.closed, a4.closed, b.closed) == (1, 1, 1)
