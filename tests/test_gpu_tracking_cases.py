"""The tracking pass (k_tracking_select, k_tracking_update, k_ever_free, the host's limit search, k_reset_inactive) on the hand-built
maps and hand-picked clocks of tests/tracking_cases.py.  After every call the device is compared with the CPU oracle -- the whole
map and its digest, the free-or-ever-free bits that only a halo export shows, the archived block lists -- and with a second context
that visits every block in every pass (disable_culling), bit for bit.  tests/test_cpu_tracking_cases.py shows on the CPU that the
maps and schedules reach what they are built to reach."""
import numpy as np
import pytest

import tracking_cases as tc
from common import assert_digests_equal, compare_maps
from khronos_amd import FusionContext, checkpoint as ck, default_config
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
VPS, NN, BASES = [8, 16], [6, 18, 26], sorted(tc.BASES)
grid = lambda f: pytest.mark.parametrize("base", BASES)(pytest.mark.parametrize("nn", NN)(pytest.mark.parametrize("vps", VPS)(f)))


def make_cfg(vps, nn, **kw):
    return default_config(max_blocks=1024, max_frame_pixels=tc.WALL_W * tc.WALL_H, exact_arithmetic=1, **tc.config(vps, nn, **kw))


class Trio:
    """the same map in a context, in a context that skips nothing, and in the oracle"""

    def __init__(self, vps, nn, indices=None, layers=None, **kw):
        self.cfg = make_cfg(vps, nn, **kw)
        self.ctx, self.all = FusionContext(self.cfg), FusionContext(make_cfg(vps, nn, disable_culling=1, **kw))
        self.ora = po.OracleMap(po.config_from(self.cfg, 0))
        self.stamp = None
        if indices is not None:
            blob = ck.pack(self.cfg, indices, layers)
            assert self.ctx.load_map(blob) == len(indices) and self.all.load_map(blob) == len(indices)
            self.ora.put_blocks(indices, layers)
            self.check("loaded", halo=False)

    def check(self, what, halo=True):
        compare_maps(self.ctx, self.ora)
        assert np.array_equal(self.ctx.block_indices(), self.all.block_indices()), what
        assert_digests_equal(self.ctx.map_digest(), self.all.map_digest(), what=("skipping vs visiting every block", what))
        if halo:   # the free-or-ever-free bits of the latest pass
            n = self.ora.num_blocks()
            want = self.ora.export_halo(self.stamp, max(1, n))[:n]
            for c in (self.ctx, self.all):
                got = c.export_halo(max(1, n))
                assert int((got[:, 1] == 1).sum()) == n, what
                assert np.array_equal(got[np.argsort(got[:n, 0])], want[np.argsort(want[:, 0])]), (what, "free bits")

    def track(self, stamp, what=""):
        self.stamp = int(stamp)
        for m in (self.ctx, self.all, self.ora):
            m.update_tracking(self.stamp)
        self.check((what, stamp))

    def reset(self, what=""):
        want = np.asarray(self.ora.reset_inactive()).reshape(-1, 3)
        for c in (self.ctx, self.all):
            assert np.array_equal(np.asarray(c.reset_inactive()).reshape(-1, 3), want), (what, "archived blocks")
        self.check((what, "reset"))
        return len(want)

    def integrate(self, sensor, stamp, depth, allocate_blocks=True, what=""):
        for c in (self.ctx, self.all):
            c.integrate(c.upload_frame(c.make_sensor(**sensor), stamp, np.eye(4), depth), allocate_blocks=allocate_blocks)
        self.ora.integrate(self.ora.make_sensor(**sensor), stamp, np.eye(4), depth, allocate_blocks=allocate_blocks)
        self.check((what, stamp, "frame"), halo=False)   # (the bits are the latest pass's: they do not know the frame yet)

    def close(self):
        for m in (self.ctx, self.all, self.ora):
            m.close()


def run_schedule(t, schedule, epoch):
    """a schedule of tracking_cases on all three; every step is held to what it was built to change, on the oracle"""
    before, stamp, removed = None, schedule[0][1], []
    for step, at in schedule:
        if at is None:
            removed.append(t.reset(step))
            before = None
            continue
        stamp = at
        t.track(stamp, step)
        after = tc.oracle_state(t.ora, stamp)
        if before is not None:
            tc.assert_step(step, epoch, before, after)
        before = after
    return removed


@grid
def test_limits_on_the_grid(vps, nn, base):
    """stamps on lim_active / lim_free and one nanosecond either side, distances on the occupancy threshold and one ulp either side;
    the same stamp twice, + 1 ns (nothing moves at the epoch base, something at the 1 s base), + 256 ns, a step across one planted
    last_occupied, a step back, a step across one planted last_observed, + 3 s; two archival calls"""
    now = tc.BASES[base]
    t = Trio(vps, nn, *tc.clock_map(vps, now))
    removed = run_schedule(t, tc.limit_schedule(now), base == "epoch")
    assert removed[0] >= 1 and sum(removed) == len(tc.CLOCK_BLOCKS) + 1 and t.ctx.num_blocks() == 0
    t.close()


@pytest.mark.parametrize("nn", NN)
@pytest.mark.parametrize("vps", VPS)
def test_small_clock(vps, nn):
    """now < temporal_window: the limit is 0 and never-observed voxels count as active, as the reference has it"""
    t = Trio(vps, nn, *tc.clock_map(vps, tc.SMALL_NOW))
    run_schedule(t, tc.small_schedule()[:1], False)
    idx = t.ctx.block_indices()
    never = sum(int(((b["last_observed"] == 0) & ((b["flags"] & tc.VOX_ACTIVE) != 0)).sum()) for b in (t.ctx.download_block(i) for i in idx))
    assert never > 100
    run_schedule(t, tc.small_schedule()[1:], False)
    assert t.ctx.num_blocks() == 0
    t.close()


@grid
def test_ever_free(vps, nn, base):
    """one pass over the free-space group with its two absent blocks; then the same map with halo records of the absent blocks
    imported on all sides.  Blocks without TRACKING_UPDATED gain no ever-free bit."""
    now = tc.BASES[base]
    idx, layers = tc.free_space_map(vps, now)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    flagged = (layers["block_flags"][order] & tc.BLK_TRACKING_UPDATED) != 0
    outcome = []
    for halo in (False, True):
        t = Trio(vps, nn, idx, layers, **(dict(rank=0, world_size=tc.FREE_WORLD) if halo else {}))
        if halo:
            recs, _ = tc.halo_records(vps)
            for m in (t.ctx, t.all, t.ora):
                m.import_halo(recs)
        t.track(now, "halo" if halo else "no halo")
        assert np.array_equal(t.ctx.block_indices(), idx[order])
        new = np.stack([t.ctx.download_block(b)["flags"] for b in idx[order]]) & ~layers["flags"][order] & tc.VOX_EVER_FREE
        assert new[flagged].any() and not new[~flagged].any()
        outcome.append(new)
        t.close()
    assert (outcome[0] != outcome[1]).sum() >= 50     # (the count test_cpu_tracking_cases.py asserts on the oracle)


@grid
def test_skips_are_real(vps, nn, base):
    """after a pass over every block, a pass whose limits cross no block's minima visits no block -- and the occupied voxels'
    last_occupied still reads as the new stamp; a pass that crosses one block's earliest not-yet-free last_occupied visits that
    block alone"""
    now = tc.BASES[base]
    idx, layers, late = tc.skip_map(vps, now)
    t = Trio(vps, nn, idx, layers)
    t.track(now, "first")
    n = len(idx)
    assert t.ctx.stats()["n_tracking_processed_blocks"] == n and t.all.stats()["n_tracking_processed_blocks"] == n
    occupied = layers["distance"] < tc.occupancy_threshold()
    assert 0.2 < occupied.mean() < 0.5
    for what, step, visited in (("quiet", tc.SKIP_QUIET, 0), ("cross", tc.SKIP_CROSS, 1)):
        bits = tc.oracle_state(t.ora, t.stamp)["free_bits"]
        t.track(now + step, what)
        assert t.ctx.stats()["n_tracking_processed_blocks"] == visited, what
        assert t.all.stats()["n_tracking_processed_blocks"] == n
        for i, b in enumerate(idx):
            got = t.ctx.download_block(b)["last_occupied"]
            assert (got[occupied[i]] == now + step).all() and (got[~occupied[i]] != now + step).all(), (what, i)
        changed = np.flatnonzero((tc.oracle_state(t.ora, t.stamp)["free_bits"] != bits).any(axis=1))
        order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
        assert [int(order[k]) for k in changed] == ([tc.SKIP_LATE_BLOCK] if visited else []), (what, changed)
    t.close()


@grid
def test_stale_neighbour(vps, nn, base):
    """block A is untouched and its face voxels become free exactly at t2; block B beside it is the only block the frame at t2
    touches: the ever-free bits on B's face towards A need A's bits of THIS pass"""
    t1 = tc.BASES[base]
    t2 = t1 + 100_000_000
    t = Trio(vps, nn, *tc.stale_pair(vps, t1, t2))
    t.track(t1, "t1")
    t.integrate(tc.STALE_SENSOR, t2, tc.stale_frame(vps), allocate_blocks=False, what="stale")
    a, b = t.ora.get_block(tc.STALE_A), t.ora.get_block(tc.STALE_B)
    assert (b["block_flags"] & tc.BLK_TRACKING_UPDATED) and not (a["block_flags"] & tc.BLK_TRACKING_UPDATED)
    t.track(t2, "t2")
    assert t.ctx.stats()["n_tracking_processed_blocks"] == 2 and t.ctx.stats()["n_tracking_updated_blocks"] == 1
    face = lambda blk: blk["flags"].reshape(vps, vps, vps)[:, :, 0] & tc.VOX_EVER_FREE
    want = face(t.ora.get_block(tc.STALE_B))
    assert want.any() and not want.all()
    assert np.array_equal(face(t.ctx.download_block(tc.STALE_B)), want) and np.array_equal(face(t.all.download_block(tc.STALE_B)), want)
    t.close()


@grid
def test_wall_walk_from_an_empty_map(vps, nn, base):
    """identity pose, 64 x 48 frames of a fronto-parallel wall that steps back three voxels per frame: occupied voxels become
    unoccupied and the previous pass's stamp is materialised.  Gaps of 0.05 s, 0.26 s and 0.8 s, two passes with no frame between
    them, a frame with no pass after it, two frames sharing one stamp."""
    t = Trio(vps, nn)
    stamp, n_pass = tc.BASES[base], 0
    for gap, what in tc.WALL_SCHEDULE:
        stamp += int(round(gap * 1e9))
        if what == "pass":
            t.track(stamp, n_pass)
            n_pass += 1
        else:
            t.integrate(tc.WALL_SENSOR, stamp, tc.wall_depth(int(what.split()[1])), what=what)
    assert 0 < t.ctx.num_blocks() < 400
    t.reset("end")
    t.close()
