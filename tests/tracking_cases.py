"""Hand-built maps and hand-picked clocks for the tracking pass (tests/test_cpu_tracking_cases.py, tests/test_gpu_tracking_cases.py):
stamps, distances and absent blocks chosen by the test instead of left behind by a stream.  Seeded, pure numpy.  Every builder
returns (indices (n, 3) int32, layers) as khronos_amd.checkpoint.pack takes them -- FusionContext.load_map(pack(...)) on the device
side, OracleMap.put_blocks(indices, layers) on the oracle side -- and `blocks_of` turns the same pair into the dictionaries of the
numpy restatement (oracle/np_oracle.tracking_pass).

Clocks: a stamp is uint64 nanoseconds and the reference compares double seconds, toSeconds(x) >= toSeconds(now) - window.
`limit(T)` is the smallest stamp on the true side of such a comparison; at the 1 s base the double of a stamp is exact and the limit
moves with every nanosecond, at the epoch base (1.7e18 ns, above 2^60) the double of a stamp is a multiple of 256 ns.

Measured with the oracle on the CPU (tests/test_cpu_tracking_cases.py prints these and asserts the conditions they have to meet):
  * clock_map, seed 5: every planted last_observed / last_occupied / distance value occurs at least 49 times in every block at
      vps 8 (60 on the 0.5 s clock) and at least 449 times at vps 16 (535).  Its first pass sets 4 (vps 8) / 33 (vps 16) new
      ever-free bits with connectivity 6 and none at all with 18 or 26 -- a random map is no test of the ever-free pass; the first
      reset_inactive archives 1 block, the one after + 3 s the other 7.
  * free_space_map, seed 5, the same counts at both clock bases (ever-free share of the voxels in TRACKING_UPDATED blocks /
      refused only by a neighbour in another present block / only by an absent block / outcome changed by halo_records):
      vps 8, 6144 voxels in 12 flagged blocks:   nn 6: 40.6 % / 122 / 1362 / 213;  nn 18: 18.7 % / 249 / 870 / 121;
                                                 nn 26: 11.8 % / 294 / 694 / 94;  outcome differs nn 6 / 18: 1341, nn 18 / 26: 425
      vps 16, 45056 voxels in 11 flagged blocks: nn 6: 54.0 % / 527 / 5446 / 914;  nn 18: 27.3 % / 1155 / 3486 / 448;
                                                 nn 26: 17.6 % / 1298 / 2782 / 251;  outcome differs nn 6 / 18: 12047, nn 18 / 26: 4351
      (without the face_occupied voxels: 46.5 % / 25.5 % / 17.4 % ever-free at vps 8, but only 81 voxels refused only by a present
      neighbour block with connectivity 6)
  * stale_pair: 32 (vps 8) / 128 (vps 16) of A's face voxels become free exactly at t2; B's face gains 16 / 6 / 6 ever-free voxels at
      vps 8 and 98 / 84 / 84 at vps 16 with connectivity 6 / 18 / 26.
  * the wall walk: 56 blocks at vps 8, 20 at vps 16; 1375 / 1207 voxels stop being occupied between two passes, 415 / 360 voxels
      are ever-free at the end.
"""
import numpy as np

f32 = np.float32
VOXEL_SIZE, TRUNCATION, NUM_LABELS = 0.1, 0.3, 3
WINDOW, BUFFER, OCC_THRESHOLD = 0.75, 0.25, -1.5
CONFIG = dict(voxel_size=VOXEL_SIZE, truncation_distance=TRUNCATION, with_semantics=1, with_tracking=1, num_labels=NUM_LABELS,
              semantic_mode=0, temporal_window=WINDOW, temporal_buffer=BUFFER, tsdf_occupancy_threshold=OCC_THRESHOLD)
BASES = {"1s": 1_000_000_000, "epoch": 1_700_000_000_123_456_789}
SMALL_NOW = 500_000_000                        # a clock that has not run for one temporal window yet
VOX_ACTIVE, VOX_EVER_FREE, VOX_TO_REMOVE, VOX_SEM_VALID = 1, 2, 4, 8
BLK_UPDATED, BLK_MESH_UPDATED, BLK_TRACKING_UPDATED, BLK_HAS_ACTIVE_DATA = 1, 2, 4, 8
SEED, DEFECT_SHARE = 5, 0.012
# steps of the limit schedule that cross one planted stamp each: last_occupied = lf + FREE_PLANT is crossed by now + FREE_STEP and
# last_observed = la + ACTIVE_PLANT by now + ACTIVE_STEP, with more than the 512 ns of the epoch clock's rounding between them
FREE_PLANT, FREE_STEP, ACTIVE_PLANT, ACTIVE_STEP = 20_000, 30_000, 50_000, 60_000


def config(vps, nn, **kw):
    return dict(CONFIG, voxels_per_side=vps, neighbor_connectivity=nn, **kw)


def np_config(vps, nn):
    """the configuration as oracle/np_oracle.py reads it"""
    return config(vps, nn)


# ---- clocks ----
def limit(T):
    """smallest integer x in [0, 2^64) with float(x) / 1e9 >= T (2^64 - 1 if there is none): x -> float(x) / 1e9 does not decrease,
    so the first x on the true side is found by bisection.  Python's own double arithmetic throughout."""
    if 0.0 / 1e9 >= T:
        return 0
    lo, hi = 0, 2 ** 64 - 1
    if not float(hi) / 1e9 >= T:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if float(mid) / 1e9 >= T:
            hi = mid
        else:
            lo = mid
    return hi


def lim_active(now, window=WINDOW):
    """first stamp that counts as active at `now` (the float32 configuration value widened to double, as the C side does)"""
    return limit(float(now) / 1e9 - float(f32(window)))


def lim_free(now, buffer=BUFFER):
    """first last_occupied stamp that is NOT free at `now`: free is the strict toSeconds(last_occupied) < toSeconds(now) - buffer"""
    return limit(float(now) / 1e9 - float(f32(buffer)))


def long_ago(now):
    return max(1, int(now) // 7)


def occupancy_threshold():
    """tests/common.occupancy_threshold in the arithmetic of the C side: float32 times float32 (the product of two float32 is exact
    in double, so rounding the double product once gives the same float32)"""
    return f32(-OCC_THRESHOLD) * f32(VOXEL_SIZE) if OCC_THRESHOLD < 0 else f32(OCC_THRESHOLD)


def planted_stamps(now):
    """(last_observed values, last_occupied values) of clock_map: name -> stamp; values that would be negative are left out"""
    la, lf = lim_active(now), lim_free(now)
    obs = {"zero": 0, "long_ago": long_ago(now), "la-1": la - 1, "la": la, "la+1": la + 1, "la+100": la + 100, "la+step": la + ACTIVE_PLANT, "now": int(now)}
    occ = {"zero": 0, "long_ago": long_ago(now), "lf-1": lf - 1, "lf": lf, "lf+1": lf + 1, "lf+100": lf + 100, "lf+step": lf + FREE_PLANT}
    return {k: v for k, v in obs.items() if v >= 0}, {k: v for k, v in occ.items() if v >= 0}


def planted_distances():
    thr = occupancy_threshold()
    return {"negative": f32(-0.2), "below": np.nextafter(thr, f32(-np.inf)), "thr": thr, "above": np.nextafter(thr, f32(np.inf)),
            "far": f32(0.29)}


# ---- maps ----
def _common_layers(rng, n, nv):
    return {"weight": rng.uniform(1.0, 2.0, (n, nv)).astype(f32), "color": rng.integers(0, 256, (n, nv, 4)).astype(np.uint8),
            "sem_label": rng.integers(0, NUM_LABELS, (n, nv)).astype(np.uint32), "likelihoods": np.zeros((n, nv, NUM_LABELS), f32)}


CLOCK_BLOCKS = [(-7, 3, -2), (-6, 3, -2), (-7, 4, -2), (-6, 4, -2), (-6, 4, -1), (40, -11, 5), (-90, 0, 17)]
CLOCK_STALE_BLOCK = (12, 12, -30)   # nothing observed inside the window: the first reset_inactive drops it


def clock_map(vps, now, seed=SEED):
    """blocks (a 2 x 2 x 1 group with a fifth on top, two isolated ones) in which every voxel draws its last_observed, last_occupied
    and distance independently from the planted values, its public flags from 0..7 (| SEM_VALID) and every block its flags from
    0..15; and one more block whose voxels were all observed before the window."""
    rng = np.random.default_rng(seed)
    nv = vps ** 3
    idx = CLOCK_BLOCKS + [CLOCK_STALE_BLOCK]
    n = len(idx)
    obs, occ = planted_stamps(now)
    dist = planted_distances()
    pick = lambda values, shape: np.array(list(values), dtype=None)[rng.integers(0, len(values), shape)]
    layers = _common_layers(rng, n, nv)
    layers["last_observed"] = pick([np.uint64(v) for v in obs.values()], (n, nv)).astype(np.uint64)
    layers["last_occupied"] = pick([np.uint64(v) for v in occ.values()], (n, nv)).astype(np.uint64)
    layers["distance"] = pick(list(dist.values()), (n, nv)).astype(f32)
    layers["flags"] = (rng.integers(0, 8, (n, nv)) | VOX_SEM_VALID).astype(np.uint8)
    layers["block_flags"] = rng.integers(0, 16, n).astype(np.uint8)
    old = [np.uint64(v) for k, v in obs.items() if k in ("zero", "long_ago", "la-1") and v < lim_active(now)] or [np.uint64(0)]
    layers["last_observed"][n - 1] = pick(old, nv).astype(np.uint64)
    layers["block_flags"][n - 1] |= BLK_HAS_ACTIVE_DATA   # it is the pass that finds the block without active data
    return np.array(idx, np.int32), layers


def owner_of(idx, world):
    """khr_device.h: ownerOf, over an (..., 3) array of block indices"""
    def mix(h):
        h = h & np.uint64(0xFFFFFFFF)
        h = h ^ (h >> np.uint64(16))
        h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
        return h ^ (h >> np.uint64(16))
    a = np.asarray(idx, np.int64)
    m32 = np.uint64(0xFFFFFFFF)
    x, y, z = ((a[..., k] & 0xFFFFFFFF).astype(np.uint64) for k in range(3))
    h = mix(((x * np.uint64(73856093)) & m32) ^ mix(((y * np.uint64(19349663)) & m32) ^ mix((z * np.uint64(83492791)) & m32)))
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


FREE_DIMS = (3, 3, 2)
FREE_ABSENT = [(1, 1, 1), (0, 2, 0)]     # beside every block of the upper layer and above the lower centre; a corner of the rim
FREE_WORLD = 2                           # the halo leg runs as rank 0 of 2: a rank imports records of the other ranks' blocks only


def free_offsets():
    present = [o for o in np.ndindex(*FREE_DIMS) if o not in FREE_ABSENT]
    return present, list(FREE_ABSENT)


def origin_ok(origin):
    """rank 0 of FREE_WORLD owns every present block of the group at `origin` and neither absent one"""
    present, absent = free_offsets()
    own = lambda offs: owner_of(np.asarray(offs) + np.asarray(origin), FREE_WORLD)
    return bool((own(present) == 0).all() and (own(absent) != 0).all())


def find_free_origin(limit_tries=1 << 22):
    """the first origin (-t, -t % 1013 - 2, -t % 97 - 3), t = 1, 2, ..., at which origin_ok holds"""
    present, absent = free_offsets()
    t = np.arange(1, limit_tries, dtype=np.int64)
    org = np.stack([-t, -(t % 1013) - 2, -(t % 97) - 3], axis=1)
    ok = np.ones(len(t), bool)
    for o in present:
        ok &= owner_of(org + np.asarray(o), FREE_WORLD) == 0
    for o in absent:
        ok &= owner_of(org + np.asarray(o), FREE_WORLD) != 0
    hit = np.flatnonzero(ok)
    assert len(hit), "no origin found"
    return tuple(int(v) for v in org[hit[0]])


FREE_ORIGIN = (-207891, -228, -23)       # find_free_origin() (seconds of search: not run on import; origin_ok is asserted)
DEFECT_KINDS = ("occupied", "occ_at_lf", "occ_before_lf", "never_observed", "ever_free_occupied", "ulp_below_thr", "at_thr")


FACE_SHARE = 0.12


def free_space_map(vps, now, seed=SEED, share=DEFECT_SHARE, updated_share=0.7, face_share=FACE_SHARE, with_plan=False):
    """a 3 x 3 x 2 group of blocks at a negative origin without the two FREE_ABSENT blocks; about 70 % of the blocks carry
    TRACKING_UPDATED.  Every voxel is observed, unoccupied and free (last_occupied well before lim_free) except for the planted
    DEFECT_KINDS, each on about `share` of the voxels -- and `face_share` more occupied voxels on the low faces (x, y or z = 0) of
    every block that have a present block beyond them ("face_occupied"): each refuses a voxel of the block beyond that face, which the uniform defects alone
    do for fewer than 100 voxels at vps 8 with connectivity 6.  plan: kind -> bool (n, nv)."""
    rng = np.random.default_rng(seed)
    nv = vps ** 3
    present, _ = free_offsets()
    idx = np.array([[FREE_ORIGIN[k] + o[k] for k in range(3)] for o in present], np.int32)
    n = len(idx)
    la, lf, thr = lim_active(now), lim_free(now), occupancy_threshold()
    layers = _common_layers(rng, n, nv)
    old_occ = np.array([0, long_ago(now), max(0, lf - 1_000_000), max(0, lf - 2)], np.uint64)
    seen = np.array([long_ago(now), max(1, la - 1), la + 1, int(now)], np.uint64)
    layers["last_occupied"] = old_occ[rng.integers(0, len(old_occ), (n, nv))]
    layers["last_observed"] = seen[rng.integers(0, len(seen), (n, nv))]
    layers["distance"] = rng.uniform(0.2, 0.3, (n, nv)).astype(f32)
    layers["flags"] = np.full((n, nv), VOX_SEM_VALID, np.uint8)
    layers["flags"][layers["last_observed"] >= np.uint64(la)] |= VOX_ACTIVE
    u = rng.random((n, nv))
    plan = {k: (u >= i * share) & (u < (i + 1) * share) for i, k in enumerate(DEFECT_KINDS)}
    layers["distance"][plan["occupied"]] = f32(-0.1)
    layers["last_occupied"][plan["occ_at_lf"]] = lf
    layers["last_occupied"][plan["occ_before_lf"]] = max(0, lf - 1)
    layers["last_observed"][plan["never_observed"]] = 0
    layers["flags"][plan["never_observed"]] &= ~np.uint8(VOX_ACTIVE)
    layers["distance"][plan["ever_free_occupied"]] = f32(0.0)
    layers["flags"][plan["ever_free_occupied"]] |= VOX_EVER_FREE
    layers["distance"][plan["ulp_below_thr"]] = np.nextafter(thr, f32(-np.inf))
    layers["distance"][plan["at_thr"]] = thr
    bfl = np.full(n, BLK_UPDATED | BLK_MESH_UPDATED | BLK_HAS_ACTIVE_DATA, np.uint8)
    bfl[rng.random(n) < updated_share] |= BLK_TRACKING_UPDATED
    layers["block_flags"] = bfl
    lin = np.arange(nv)
    planes = [lin % vps == 0, (lin // vps) % vps == 0, lin // (vps * vps) == 0]
    low = np.zeros((n, nv), bool)
    for i, o in enumerate(present):      # the low faces with a present block beyond them
        for k in range(3):
            beyond = tuple(o[a] - (a == k) for a in range(3))
            if beyond in present:
                low[i] |= planes[k]
    plan["face_occupied"] = low & (rng.random((n, nv)) < face_share) & (u >= len(DEFECT_KINDS) * share)
    layers["distance"][plan["face_occupied"]] = f32(-0.1)
    return (idx, layers, plan) if with_plan else (idx, layers)


def pack_key(b):
    """khr_device.h: packKey -- 21 bits per coordinate, offset by 2^20"""
    return sum(((int(b[k]) + (1 << 20)) & 0x1FFFFF) << (21 * k) for k in range(3))


def halo_records(vps, seed=SEED, ones=0.95, blocks=None):
    """66-word records (key, valid = 1, 64 words of free-or-ever-free bits; a block of vps 8 uses the first 8) of the absent blocks
    of free_space_map, a bit set with probability `ones`; and the same bits as {block index: bool (nv,)} for the numpy side"""
    rng = np.random.default_rng(seed + 77)
    if blocks is None:
        blocks = [tuple(FREE_ORIGIN[k] + o[k] for k in range(3)) for o in FREE_ABSENT]
    nv = vps ** 3
    recs = np.zeros((len(blocks), 66), np.uint64)
    bits = {}
    for i, b in enumerate(blocks):
        v = rng.random(4096) < ones
        recs[i, 0], recs[i, 1] = pack_key(b), 1
        recs[i, 2:] = np.packbits(v, bitorder="little").view(np.uint64)
        bits[tuple(b)] = v[:nv].copy()
    return recs, bits


def blocks_of(indices, layers):
    """the map as oracle/np_oracle.tracking_pass takes it: {(bx, by, bz): dict(dist, last_obs, last_occ, flags, block_flags)}, copies"""
    return {tuple(int(v) for v in b): dict(dist=layers["distance"][i].copy(), last_obs=layers["last_observed"][i].copy(),
                                           last_occ=layers["last_occupied"][i].copy(), flags=layers["flags"][i].copy(),
                                           block_flags=int(layers["block_flags"][i]))
            for i, b in enumerate(np.asarray(indices).reshape(-1, 3))}


# ---- the stale neighbour: block A beside block B, a frame that touches B alone ----
STALE_A, STALE_B = (-1, 0, 1), (0, 0, 1)
STALE_SENSOR = dict(width=32, height=24, fx=20.0, fy=20.0, cx=16.0, cy=12.0)


def stale_pair(vps, t1, t2, seed=SEED):
    """A and B, every voxel observed, unoccupied, and free long before t1 -- except A's face towards B (x = vps - 1): there
    last_occupied is lf(t2) - 1 (free exactly from t2 on) in the lower half (y) and lf(t2) (not yet) in the upper."""
    rng = np.random.default_rng(seed + 1)
    nv = vps ** 3
    assert lim_free(t2) - 1 >= lim_free(t1)          # A's face is not free at t1
    layers = _common_layers(rng, 2, nv)
    layers["distance"] = rng.uniform(0.2, 0.3, (2, nv)).astype(f32)
    layers["last_observed"] = np.full((2, nv), int(t1), np.uint64)
    layers["last_occupied"] = np.full((2, nv), long_ago(t1), np.uint64)
    layers["flags"] = np.full((2, nv), VOX_SEM_VALID | VOX_ACTIVE, np.uint8)
    layers["block_flags"] = np.full(2, BLK_HAS_ACTIVE_DATA, np.uint8)
    lin = np.arange(nv)
    x, y, z = lin % vps, (lin // vps) % vps, lin // (vps * vps)
    face = x == vps - 1
    lf2 = lim_free(t2)
    layers["last_occupied"][0][face & (y < vps // 2)] = lf2 - 1
    layers["last_occupied"][0][face & (y >= vps // 2)] = lf2
    return np.array([STALE_A, STALE_B], np.int32), layers


def stale_frame(vps):
    """depth image of STALE_SENSOR at the identity pose: a wall through the middle of the blocks' z range, seen only by the columns
    whose rays stay more than two pixels on B's side of x = 0 (A's voxels never read a valid pixel)"""
    w, h = STALE_SENSOR["width"], STALE_SENSOR["height"]
    depth = np.zeros((h, w), f32)
    depth[:, int(STALE_SENSOR["cx"]) + 3:] = f32(1.5 * vps * VOXEL_SIZE)
    return depth


# ---- the wall walk ----
WALL_W, WALL_H = 64, 48
WALL_SENSOR = dict(width=WALL_W, height=WALL_H, fx=60.0, fy=60.0, cx=31.5, cy=23.5, min_range=0.1, max_range=2.6)
# (seconds since the previous event, what happens): "frame k" integrates a fronto-parallel wall at 0.9 m + 3 voxels * k, "pass" runs
# the tracking pass at the current stamp.  Gaps of 0.05 s, 0.26 s (just over the buffer) and 0.8 s (just over the window); two passes
# with no frame between them, a frame with no pass after it, two frames sharing one stamp.
WALL_SCHEDULE = [(0.0, "frame 0"), (0.0, "pass"), (0.05, "frame 1"), (0.0, "pass"), (0.05, "frame 2"), (0.05, "frame 3"), (0.0, "pass"),
                 (0.26, "pass"), (0.05, "pass"), (0.26, "frame 4"), (0.0, "frame 2"), (0.0, "pass"), (0.8, "frame 5"), (0.0, "pass"),
                 (0.8, "pass")]


def wall_depth(k):
    return np.full((WALL_H, WALL_W), f32(0.9) + f32(3 * VOXEL_SIZE) * f32(k), f32)


# ---- schedules and what the oracle shows of a map ----
def limit_schedule(now):
    """[(step, stamp)] of the limit test; a "reset" step (stamp None) calls reset_inactive"""
    return [("first", now), ("same", now), ("+1ns", now + 1), ("+256ns", now + 256), ("reset", None), ("free", now + FREE_STEP),
            ("back", now - 100_000_000), ("active", now + ACTIVE_STEP), ("+3s", now + 3_000_000_000), ("reset", None)]


def small_schedule():
    """now < window: the limit is 0 and never-observed voxels count as active; then the window opens, then everything ages out"""
    return [("first", SMALL_NOW), ("same", SMALL_NOW), ("opens", SMALL_NOW + 300_000_000), ("+3s", SMALL_NOW + 3_000_000_000), ("reset", None)]


def oracle_state(ora, stamp):
    """everything a tracking pass can change, of every block of an OracleMap: voxel flags, block flags, last_occupied and the
    free-or-ever-free bits at `stamp` (which no download shows: they go to the other ranks, OracleMap.export_halo)"""
    idx = ora.block_indices().copy()
    blocks = [ora.get_block(b, likelihoods=False) for b in idx]
    nv = ora.nvox
    stack = lambda k, dt: np.stack([b[k] for b in blocks]) if blocks else np.zeros((0, nv), dt)
    return dict(indices=idx, flags=stack("flags", np.uint8), last_occupied=stack("last_occupied", np.uint64),
                last_observed=stack("last_observed", np.uint64), distance=stack("distance", f32),
                block_flags=np.array([b["block_flags"] for b in blocks], np.uint8),
                free_bits=ora.export_halo(stamp, max(1, len(idx)))[:len(idx), 2:2 + max(1, nv // 64)].copy())


def assert_step(step, epoch, before, after):
    """every pass of a schedule changes what the step was built to change, and the steps built to change nothing change nothing"""
    same = lambda k: np.array_equal(before[k], after[k])
    if step == "same":
        assert all(same(k) for k in before), step
    elif step == "+1ns" and epoch:   # the double of the stamp does not move: no limit moves (an occupied voxel's last_occupied does)
        assert same("flags") and same("block_flags") and same("free_bits"), step
        assert not same("last_occupied")
    elif step == "free":
        assert same("flags") and same("block_flags") and not same("free_bits"), step
    elif step in ("+1ns", "+256ns", "back", "active", "opens", "+3s"):
        assert same("indices") and not same("flags"), step
    if step == "+3s":
        assert not (after["flags"] & VOX_ACTIVE).any() and not (after["block_flags"] & BLK_HAS_ACTIVE_DATA).any()


# ---- skips ----
SKIP_BLOCKS = [(5, -3, 2), (6, -3, 2), (5, -2, 2), (-20, 9, 0)]
SKIP_LATE_BLOCK, SKIP_PLANT, SKIP_QUIET, SKIP_CROSS = 2, 1_000_000, 500_000, 2_000_000


def skip_map(vps, now, seed=SEED):
    """blocks in which nothing can change for a while after a pass at `now`: every voxel observed at `now`; a third of them occupied
    (their last_occupied is the stamp of every pass, which the device does not store), the others free long ago -- except one
    voxel of block SKIP_LATE_BLOCK whose last_occupied is lf(now) + SKIP_PLANT: a pass at now + SKIP_QUIET crosses no block's minima,
    one at now + SKIP_CROSS crosses that block's earliest not-yet-free last_occupied and nothing else."""
    rng = np.random.default_rng(seed + 2)
    n, nv = len(SKIP_BLOCKS), vps ** 3
    layers = _common_layers(rng, n, nv)
    occupied = rng.random((n, nv)) < 1 / 3
    layers["distance"] = np.where(occupied, f32(0.05), f32(0.25)).astype(f32)
    layers["last_observed"] = np.full((n, nv), int(now), np.uint64)
    layers["last_occupied"] = np.full((n, nv), long_ago(now), np.uint64)
    layers["flags"] = np.full((n, nv), VOX_SEM_VALID | VOX_ACTIVE, np.uint8)
    layers["block_flags"] = np.full(n, BLK_HAS_ACTIVE_DATA | BLK_TRACKING_UPDATED, np.uint8)
    late = int(np.flatnonzero(~occupied[SKIP_LATE_BLOCK])[nv // 5])
    layers["last_occupied"][SKIP_LATE_BLOCK, late] = lim_free(now) + SKIP_PLANT
    assert lim_free(now + SKIP_QUIET) <= lim_free(now) + SKIP_PLANT < lim_free(now + SKIP_CROSS) and lim_active(now + SKIP_CROSS) <= now
    return np.array(SKIP_BLOCKS, np.int32), layers, late
