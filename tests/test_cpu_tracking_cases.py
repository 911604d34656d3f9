"""The maps and clocks of tests/tracking_cases.py on the CPU: the oracle's tracking pass (orc_update_tracking, orc_reset_inactive,
orc_import_halo) is held to the numpy restatement (oracle/np_oracle.tracking_pass) on every map and schedule the device test uses
and, where the state is reachable through the reference's own integrator, to the compiled reference; and the maps are shown to
contain what they were built to contain (the coverage conditions, asserted on the oracle alone; the counts are printed)."""
import numpy as np
import pytest

import tracking_cases as tc
from khronos_amd import default_config
from oracle import np_oracle as npo
from oracle import pyoracle as po
from oracle import pyref

LIB = pyref.load()
needs_ref = pytest.mark.skipif(LIB is None, reason="oracle/_ref/libref_khronos.so absent and no /root/reference to build it from")
VPS, NN, BASES = [8, 16], [6, 18, 26], sorted(tc.BASES)


def orc_cfg(vps, nn, **kw):
    return po.config_from(default_config(max_blocks=64, max_frame_pixels=64 * 48, **tc.config(vps, nn, **kw)), 0)


def oracle_with(vps, nn, indices, layers, **kw):
    ora = po.OracleMap(orc_cfg(vps, nn, **kw))
    ora.put_blocks(indices, layers)
    return ora


def assert_equals_numpy(ora, blocks, what):
    idx = [tuple(int(v) for v in b) for b in ora.block_indices()]
    assert idx == sorted(blocks), what
    for b in idx:
        o, n = ora.get_block(b, likelihoods=False), blocks[b]
        assert np.array_equal(o["last_occupied"], n["last_occ"]), (what, b, "last_occupied")
        assert np.array_equal(o["flags"], n["flags"]), (what, b, "flags", np.flatnonzero(o["flags"] != n["flags"])[:8])
        assert o["block_flags"] == n["block_flags"], (what, b, "block_flags", o["block_flags"], n["block_flags"])


def run_schedule(vps, nn, indices, layers, schedule, epoch):
    """the schedule on the oracle and in numpy, compared after every call; returns the oracle's state after each step"""
    ora, blocks, cfg = oracle_with(vps, nn, indices, layers), tc.blocks_of(indices, layers), tc.np_config(vps, nn)
    stamp, states = schedule[0][1], []
    for step, at in schedule:
        if at is None:
            gone = ora.reset_inactive()
            assert [tuple(g) for g in gone.tolist()] == npo.reset_inactive(blocks), step
            states.append((step, len(gone)))
            continue
        before = tc.oracle_state(ora, stamp) if states else None
        stamp = at
        ora.update_tracking(stamp)
        npo.tracking_pass(cfg, blocks, stamp)
        assert_equals_numpy(ora, blocks, (step, stamp))
        after = tc.oracle_state(ora, stamp)
        if before is not None:
            tc.assert_step(step, epoch, before, after)
        states.append((step, after))
    return states


# ---- clocks ----
@pytest.mark.parametrize("now", [tc.BASES["1s"], tc.BASES["epoch"], tc.SMALL_NOW, tc.BASES["epoch"] + 255, 2 ** 53 + 1, 3])
def test_limit_is_the_first_stamp_on_the_true_side(now):
    for width in (tc.WINDOW, tc.BUFFER, 3.0):
        T = float(now) / 1e9 - float(np.float32(width))
        lim = tc.limit(T)
        for x in range(max(0, lim - 700), lim + 700):
            assert (float(x) / 1e9 >= T) == (x >= lim), (now, width, x, lim)
        assert lim > 0 or T <= 0.0
    assert tc.lim_active(now) <= tc.lim_free(now) <= now


def test_epoch_clock_is_quantised():
    e = tc.BASES["epoch"]
    assert e > 2 ** 53 and (e >> 32) != 0
    assert tc.lim_active(e + 1) == tc.lim_active(e) and tc.lim_free(e + 1) == tc.lim_free(e)
    assert tc.lim_active(e + 256) > tc.lim_active(e) + 1 and tc.lim_free(e + 256) > tc.lim_free(e) + 1
    s = tc.BASES["1s"]
    assert tc.lim_active(s + 1) > tc.lim_active(s) and tc.lim_free(s + 1) > tc.lim_free(s)   # (by 1 or 2: the difference is rounded)
    for now in (e, s):   # each built step crosses its planted stamp and only that one
        la, lf = tc.lim_active, tc.lim_free
        assert la(now + 1) <= la(now) + 100 < la(now + 256) and lf(now + 1) <= lf(now) + 100 < lf(now + 256)
        assert lf(now + 256) <= lf(now) + tc.FREE_PLANT < lf(now + tc.FREE_STEP) and la(now + tc.FREE_STEP) <= la(now) + tc.ACTIVE_PLANT
        assert la(now) + tc.ACTIVE_PLANT < la(now + tc.ACTIVE_STEP)
    assert np.float32(-tc.OCC_THRESHOLD * float(np.float32(tc.VOXEL_SIZE))) == tc.occupancy_threshold()


# ---- clock_map: planted values, the limit schedule ----
@pytest.mark.parametrize("now", [tc.BASES["1s"], tc.BASES["epoch"], tc.SMALL_NOW])
@pytest.mark.parametrize("vps", VPS)
def test_clock_map_holds_every_planted_value(vps, now):
    idx, layers = tc.clock_map(vps, now)
    obs, occ = tc.planted_stamps(now)
    least = {}
    for name, values, layer in (("last_observed", obs, "last_observed"), ("last_occupied", occ, "last_occupied"),
                                ("distance", tc.planted_distances(), "distance")):
        for k, v in values.items():
            per_block = (layers[layer][:len(tc.CLOCK_BLOCKS)] == v).sum(axis=1)
            least[name + ":" + k] = int(per_block.min())
    print("clock_map vps %d now %d: fewest voxels per block and planted value %d (%s)" % (vps, now, min(least.values()), min(least, key=least.get)))
    assert min(least.values()) >= 20, least
    assert set(np.unique(layers["flags"]).tolist()) == set(range(8, 16)) and (layers["block_flags"] < 16).all()
    assert len(set(layers["block_flags"][:len(tc.CLOCK_BLOCKS)].tolist())) > 3


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("nn", NN)
@pytest.mark.parametrize("vps", VPS)
def test_limit_schedule(vps, nn, base):
    now = tc.BASES[base]
    idx, layers = tc.clock_map(vps, now)
    states = run_schedule(vps, nn, idx, layers, tc.limit_schedule(now), base == "epoch")
    resets = [s[1] for s in states if s[0] == "reset"]
    first = states[0][1]
    # the first pass hits every branch: occupied or not on either side of the threshold, active / inactive, newly to_remove,
    # new ever-free voxels in the blocks that were flagged, none in the others
    d, thr = first["distance"], tc.occupancy_threshold()
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    assert np.array_equal(first["indices"], idx[order])
    assert (first["last_occupied"][d < thr] == now).all() and (first["last_occupied"][d >= thr] != now).all()
    assert (d == thr).sum() > 100 and (d == np.nextafter(thr, np.float32(-1))).sum() > 100
    was = layers["flags"][order]
    flagged = (layers["block_flags"][order] & tc.BLK_TRACKING_UPDATED) != 0
    new_ever = ((first["flags"] & ~was) & tc.VOX_EVER_FREE) != 0
    assert not new_ever[~flagged].any() and 0 < flagged.sum() < len(idx)
    assert (((first["flags"] & ~was) & tc.VOX_TO_REMOVE) != 0).sum() > 100
    print("limit schedule vps %d nn %d %s: %d new ever-free voxels in %d flagged blocks at the first pass, archived %s"
          % (vps, nn, base, int(new_ever.sum()), int(flagged.sum()), resets))
    assert resets[0] >= 1 and resets[1] == len(idx) - resets[0], resets   # the stale block first; everything after + 3 s


@pytest.mark.parametrize("nn", NN)
@pytest.mark.parametrize("vps", VPS)
def test_small_clock(vps, nn):
    idx, layers = tc.clock_map(vps, tc.SMALL_NOW)
    assert tc.lim_active(tc.SMALL_NOW) == 0
    states = run_schedule(vps, nn, idx, layers, tc.small_schedule(), False)
    first, opened = states[0][1], states[2][1]
    never = first["last_observed"] == 0
    assert never.sum() > 100 and (first["flags"][never] & tc.VOX_ACTIVE).all()     # 0 s >= a negative limit: active
    assert not (opened["flags"][never] & tc.VOX_ACTIVE).any() and (opened["flags"][never] & tc.VOX_TO_REMOVE).all()


# ---- free_space_map: the ever-free pass and what the scene contains ----
def ever_free_outcome(vps, nn, idx, layers, now, halo=None, **kw):
    """(new ever-free bits (n, nv) of the blocks in index order, the oracle's flags) of one pass on the oracle; the numpy leg is
    compared on the way"""
    ora, blocks = oracle_with(vps, nn, idx, layers, **kw), tc.blocks_of(idx, layers)
    bits = None
    if halo is not None:
        recs, bits = halo
        ora.import_halo(recs)
    ora.update_tracking(now)
    npo.tracking_pass(tc.np_config(vps, nn), blocks, now, halo=bits)
    assert_equals_numpy(ora, blocks, ("free_space_map", vps, nn, now))
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    after = tc.oracle_state(ora, now)["flags"]
    out = np.zeros_like(after)
    out[order] = after     # back to the builder's block order
    return ((out & ~layers["flags"]) & tc.VOX_EVER_FREE) != 0


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("vps", VPS)
def test_free_space_map_coverage(vps, base):
    assert tc.origin_ok(tc.FREE_ORIGIN) and all(v < 0 for v in tc.FREE_ORIGIN)
    now = tc.BASES[base]
    idx, layers, plan = tc.free_space_map(vps, now, with_plan=True)
    nv = vps ** 3
    flagged = (layers["block_flags"] & tc.BLK_TRACKING_UPDATED) != 0
    n_in = int(flagged.sum()) * nv
    assert len(idx) == 16 and 0.5 < flagged.mean() < 0.9
    for k in tc.DEFECT_KINDS:
        assert 0.008 < plan[k].mean() < 0.016, (k, plan[k].mean())
    new = {nn: ever_free_outcome(vps, nn, idx, layers, now) for nn in NN}
    halo = tc.halo_records(vps)
    new_halo = {nn: ever_free_outcome(vps, nn, idx, layers, now, halo=halo, rank=0, world_size=tc.FREE_WORLD) for nn in NN}
    # hypothetical passes in numpy (held to the oracle above): what only the other present blocks, only the absent blocks refuse
    blocks = tc.blocks_of(idx, layers)
    cfg = tc.np_config(vps, 6)
    for d in blocks.values():
        npo.tracking_block(cfg, d["dist"], d["last_obs"], d["last_occ"], d["flags"], now)
    F, free = npo.free_or_ever_free(cfg, blocks, now)
    line = []
    for nn in NN:
        assert not new[nn][~flagged].any() and not new_halo[nn][~flagged].any()     # blocks without TRACKING_UPDATED gain no bit
        share = new[nn].sum() / n_in
        only_present = only_absent = 0
        for i, b in enumerate(idx):
            if not flagged[i]:
                continue
            b = tuple(int(v) for v in b)
            cand = free[b] & ((layers["flags"][i] & tc.VOX_EVER_FREE) == 0)
            real = npo.neighbours_ok(npo.padded_neighbourhood(F, b, vps), vps, nn)
            assert np.array_equal(cand & real, new[nn][i])
            only_present += int((cand & ~real & npo.neighbours_ok(npo.padded_neighbourhood(F, b, vps, others=True), vps, nn)).sum())
            only_absent += int((cand & ~real & npo.neighbours_ok(npo.padded_neighbourhood(F, b, vps, absent=True), vps, nn)).sum())
        by_halo = int((new[nn] != new_halo[nn]).sum())
        line.append("nn %d: %.1f %% ever-free, refused only by a present neighbour block %d, only by an absent block %d, changed by the halo %d"
                    % (nn, 100 * share, only_present, only_absent, by_halo))
        assert 0.05 <= share <= 0.80, (nn, share)
        assert only_present >= 100 and only_absent >= 100 and by_halo >= 50, line[-1]
    d1, d2 = int((new[6] != new[18]).sum()), int((new[18] != new[26]).sum())
    print("free_space_map vps %d %s, %d voxels in %d flagged blocks: %s; outcome differs nn 6 / 18: %d, nn 18 / 26: %d"
          % (vps, base, n_in, int(flagged.sum()), "; ".join(line), d1, d2))
    assert min(d1, d2) >= (300 if vps == 8 else 2000), (d1, d2)
    # the boundary defects decide as planted: last_occupied == lf is not free, lf - 1 is, distance == thr is not occupied
    state = oracle_with(vps, 6, idx, layers)
    state.update_tracking(now)
    bits = tc.oracle_state(state, now)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    free_bit = np.zeros((len(idx), nv), bool)
    free_bit[order] = np.unpackbits(bits["free_bits"].view(np.uint8), bitorder="little").reshape(len(idx), -1)[:, :nv].astype(bool)
    assert not free_bit[plan["occ_at_lf"]].any() and free_bit[plan["occ_before_lf"]].all() and free_bit[plan["at_thr"]].all()
    assert not free_bit[plan["ulp_below_thr"]].any() and not free_bit[plan["never_observed"]].any() and not free_bit[plan["occupied"] | plan["face_occupied"]].any()
    assert free_bit[plan["ever_free_occupied"]].all()


# ---- the stale neighbour and the wall walk on the oracle and in numpy (the device test runs the same scenes) ----
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("nn", NN)
@pytest.mark.parametrize("vps", VPS)
def test_stale_neighbour(vps, nn, base):
    t1 = tc.BASES[base]
    t2 = t1 + 100_000_000
    idx, layers = tc.stale_pair(vps, t1, t2)
    ora = oracle_with(vps, nn, idx, layers)
    ora.update_tracking(t1)
    sen = ora.make_sensor(**tc.STALE_SENSOR)
    ora.integrate(sen, t2, np.eye(4), tc.stale_frame(vps), allocate_blocks=False)
    a, b = ora.get_block(tc.STALE_A, likelihoods=False), ora.get_block(tc.STALE_B, likelihoods=False)
    assert (b["block_flags"] & tc.BLK_TRACKING_UPDATED) and not (a["block_flags"] & tc.BLK_TRACKING_UPDATED)
    assert np.array_equal(a["distance"], layers["distance"][0]) and np.array_equal(a["last_observed"], layers["last_observed"][0])
    assert not ((a["flags"] | b["flags"]) & tc.VOX_EVER_FREE).any()
    # numpy: the same pass from the oracle's state after the frame
    blocks = {k: dict(dist=v["distance"].copy(), last_obs=v["last_observed"].copy(), last_occ=v["last_occupied"].copy(),
                      flags=v["flags"].copy(), block_flags=v["block_flags"]) for k, v in ((tc.STALE_A, a), (tc.STALE_B, b))}
    ora.update_tracking(t2)
    npo.tracking_pass(tc.np_config(vps, nn), blocks, t2)
    assert_equals_numpy(ora, blocks, "stale neighbour")
    after = ora.get_block(tc.STALE_B, likelihoods=False)["flags"].reshape(vps, vps, vps)     # [z, y, x]
    face = (after[:, :, 0] & tc.VOX_EVER_FREE) != 0                                           # B's face towards A
    lf2 = tc.lim_free(t2)
    a_free = (layers["last_occupied"][0].reshape(vps, vps, vps)[:, :, vps - 1] < lf2)
    print("stale neighbour vps %d nn %d %s: %d ever-free voxels on B's face, %d of A's face voxels free from t2 on"
          % (vps, nn, base, int(face.sum()), int(a_free.sum())))
    assert 0 < a_free.sum() < vps * vps and face.sum() > 0 and not face[~a_free].any()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("vps", VPS)
def test_wall_walk_materialises_last_occupied(vps, base):
    """occupied voxels stop being occupied when the wall steps back: their last_occupied stays at the stamp of the last pass that
    saw them occupied -- the value the device has to materialise"""
    ora = po.OracleMap(orc_cfg(vps, 18))
    sen = ora.make_sensor(**tc.WALL_SENSOR)
    stamp, passes, released = tc.BASES[base], [], 0
    thr = tc.occupancy_threshold()
    for gap, what in tc.WALL_SCHEDULE:
        stamp += int(round(gap * 1e9))
        if what == "pass":
            before = tc.oracle_state(ora, stamp)
            ora.update_tracking(stamp)
            after = tc.oracle_state(ora, stamp)
            if passes:
                gone = (before["last_occupied"] == passes[-1]) & (after["distance"] >= thr) & (passes[-1] != stamp)
                assert (after["last_occupied"][gone] == passes[-1]).all()
                released += int(gone.sum())
            passes.append(stamp)
        else:
            ora.integrate(sen, stamp, np.eye(4), tc.wall_depth(int(what.split()[1])))
    n_ever = int(((after["flags"] & tc.VOX_EVER_FREE) != 0).sum())
    print("wall walk vps %d %s: %d blocks, %d voxels released from occupancy over %d passes, %d ever-free at the end"
          % (vps, base, len(after["indices"]), released, len(passes), n_ever))
    assert released >= 100 and n_ever >= 100 and len(after["indices"]) < 400


# ---- the compiled reference, where its own integrator can reach the state ----
@needs_ref
@pytest.mark.parametrize("base", BASES + ["small"])
@pytest.mark.parametrize("nn", NN)
@pytest.mark.parametrize("vps", VPS)
def test_schedules_against_the_reference(vps, nn, base):
    """distance, last_observed and tracking_updated of clock_map and free_space_map put into the reference's map (its tracking
    state starts empty and only its TrackingIntegrator writes it), then the schedules: the oracle follows it stamp for stamp"""
    now = tc.SMALL_NOW if base == "small" else tc.BASES[base]
    schedule = tc.small_schedule() if base == "small" else tc.limit_schedule(now)
    for name, (idx, layers) in (("clock_map", tc.clock_map(vps, now)), ("free_space_map", tc.free_space_map(vps, now))):
        cfg = orc_cfg(vps, nn)
        ora, ref = po.OracleMap(cfg), pyref.RefMap(LIB, cfg)
        for i, b in enumerate(idx):
            upd = int(layers["block_flags"][i]) & tc.BLK_TRACKING_UPDATED
            ora.put_block(b, dict(distance=layers["distance"][i], last_observed=layers["last_observed"][i], block_flags=upd))
            ref.put_block(b, layers["distance"][i], layers["last_observed"][i], upd)
        n_ever = 0
        for step, at in schedule:
            if at is None:
                assert np.array_equal(np.asarray(ora.reset_inactive()).reshape(-1, 3), ref.reset_inactive()), (name, step)
            else:
                ora.update_tracking(at)
                ref.update_tracking(at)
            assert np.array_equal(ora.block_indices(), ref.block_indices()), (name, step)
            for b in ora.block_indices():
                a, e = ora.get_block(b, likelihoods=False), ref.get_block(b)
                assert np.array_equal(a["last_observed"], e["last_observed"]), (name, step, tuple(b))
                assert np.array_equal(a["last_occupied"], e["last_occupied"]), (name, step, tuple(b), "last_occupied")
                assert np.array_equal(a["flags"] & 7, e["flags"]), (name, step, tuple(b), "active / ever_free / to_remove")
                assert (a["block_flags"] & 12) == e["block_flags"], (name, step, tuple(b), "tracking_updated / has_active_data")
                n_ever += int(((e["flags"] & 2) != 0).sum())
        if name == "free_space_map" and base != "small":
            assert n_ever > 0
