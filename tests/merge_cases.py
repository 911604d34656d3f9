"""Hand-built maps for khr_merge_map (ASSUMPTIONS.md A.17): small (indices, layers) pairs in the form of khronos_amd.checkpoint,
fixed seeds, at most about 30 blocks each.  Every voxel layer of a `rich` block draws from a short list of values chosen so that
each rule of A.17 meets each of its cases many times per block: weights {0, min_weight, the float below it, ..., half of
max_weight (a sum exactly at the cap), nearly max_weight (a sum above it)}, alpha {0, 255}, all sixteen voxel flag words
(SEM_VALID x the three tracking bits), stamps from a small range (either side may be the later one), small integer likelihoods
(tied row sums).  Needs no device."""
import numpy as np

from khronos_amd import checkpoint as ck

f32 = np.float32
MIN_WEIGHT, MAX_WEIGHT = f32(0.5), f32(10.0)
CFG16 = dict(voxel_size=0.1, voxels_per_side=16, truncation_distance=0.3, with_semantics=1, with_tracking=1, num_labels=5, semantic_mode=0)
CFG8 = dict(voxel_size=0.05, voxels_per_side=8, truncation_distance=0.15, with_semantics=1, with_tracking=1, num_labels=2, semantic_mode=1)
WEIGHTS = np.array([0, 0, MIN_WEIGHT, np.nextafter(MIN_WEIGHT, f32(0)), 1.0, 2.5, MAX_WEIGHT / 2, MAX_WEIGHT - 1], f32)


def empty_layers(cfg, n=0):
    f = ck.config_fields(cfg)
    return {k: np.zeros(sh[0], ck._DTYPES[k]) for k, sh in ck._shapes(f, n).items() if sh is not None and k != "indices"}


def rich_map(cfg, blocks, seed, color=True, weights=WEIGHTS):
    """blocks: list of (index, kind); kind "rich", "zero" (all weights 0, the other layers rich) or "solid" (all weights 2.5)"""
    rng = np.random.default_rng(seed)
    f = ck.config_fields(cfg)
    n, nv, K = len(blocks), f["voxels_per_side"] ** 3, f["num_labels"]
    L = empty_layers(cfg, n)
    idx = np.array([b for b, _ in blocks], np.int32).reshape(-1, 3)
    trunc = f32(f["truncation_distance"])
    for i, (_, kind) in enumerate(blocks):
        L["distance"][i] = rng.uniform(-trunc, trunc, nv).astype(f32)
        L["weight"][i] = {"rich": rng.choice(weights, nv), "zero": np.zeros(nv, f32), "solid": np.full(nv, 2.5, f32)}[kind]
        if color:
            L["color"][i] = rng.integers(0, 256, (nv, 4), dtype=np.uint8)
            L["color"][i][:, 3] = rng.choice(np.array([0, 255], np.uint8), nv)
        L["flags"][i] = rng.integers(0, 16, nv, dtype=np.uint8)
        L["last_observed"][i] = rng.integers(1, 40, nv).astype(np.uint64) * np.uint64(50_000_000)
        L["last_occupied"][i] = rng.integers(0, 40, nv).astype(np.uint64) * np.uint64(50_000_000)
        L["sem_label"][i] = rng.integers(0, K, nv, dtype=np.uint32)
        sv = (L["flags"][i] & 8) != 0
        L["likelihoods"][i] = np.where(sv[:, None], rng.integers(-3, 4, (nv, K)).astype(f32), f32(0))
        L["block_flags"][i] = rng.integers(0, 16)
    return idx, L


def ragged_map(cfg, blocks, seed):
    """a linear distance field inside the band, observed on a ragged region: weight 2 on nine voxels in ten, else 0"""
    idx, L = rich_map(cfg, [(b, "solid") for b in blocks], seed)
    f = ck.config_fields(cfg)
    vps, vs = f["voxels_per_side"], f32(f["voxel_size"])
    lin = np.arange(vps ** 3)
    holes = np.random.default_rng(seed + 1000)
    for i, b in enumerate(idx):
        g = [int(b[a]) * vps + (lin // vps ** a) % vps for a in range(3)]
        c = [(ga.astype(f32) + f32(0.5)) * vs for ga in g]
        L["distance"][i] = (f32(0.05) * c[0] - f32(0.03) * c[1] + f32(0.04) * c[2] - f32(0.02)).astype(f32)
        L["weight"][i] = np.where(holes.random(vps ** 3) < 0.9, f32(2), f32(0))  # 0.9^8: under half of the centres see 8 valid taps
    return idx, L


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(axis, deg), t
    return T


def _aligned(name, cfg, offset, dst_blocks, src_blocks, seed, color=True):
    d, s = rich_map(cfg, dst_blocks, seed, color), rich_map(cfg, src_blocks, seed + 1, color)
    return dict(name=name, cfg=cfg, dst=d, src=s, mode=0, voxel_offset=offset, pose=None, min_weight=float(MIN_WEIGHT))


R = "rich"
CASES = [
    # both observed / block present, voxel unobserved / block absent; a source block of zero weights far away (allocates
    # nothing); a destination block nothing reaches (3, 3, 3)
    _aligned("zero_offset", CFG16, (0, 0, 0), [((0, 0, 0), R), ((1, 0, 0), R), ((3, 3, 3), R), ((0, 1, 0), "zero")],
             [((0, 0, 0), R), ((1, 0, 0), R), ((0, 0, 1), R), ((0, 1, 0), R), ((-5, 2, 2), "zero")], 100),
    _aligned("block_offset", CFG16, (16, 0, -16), [((1, 0, -1), R), ((2, 0, 0), R), ((7, 7, 7), R)],
             [((0, 0, 0), R), ((1, 0, 0), R), ((1, 0, 1), R), ((9, 9, 9), "zero")], 200),
    _aligned("odd_offset", CFG16, (5, -3, 17), [((0, 0, 0), R), ((-1, -1, 0), R), ((0, -1, 1), "zero"), ((6, 6, 6), R)],
             [((-1, -1, -1), R), ((0, 0, 0), R), ((-2, 0, -1), R), ((4, -4, 4), "zero")], 300),
    _aligned("binary_vps8", CFG8, (3, 0, -9), [((0, 0, 0), R), ((0, 0, -1), R), ((-1, 0, -2), R), ((5, 5, 5), R)],
             [((-1, -1, -1), R), ((0, 0, 0), R), ((0, 0, 1), R), ((-1, 0, 0), R), ((8, 8, 8), "zero")], 400, color=False),
    _aligned("into_empty", CFG16, (0, 0, 0), [], [((0, 0, 0), R), ((-1, 2, 0), R)], 500),
    dict(name="resample", cfg=CFG16, dst=rich_map(CFG16, [((0, 0, 0), R), ((1, 0, 0), "zero"), ((-4, 4, 4), R)], 600),
         src=ragged_map(CFG16, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (-1, 0, 0)], 601), mode=1, voxel_offset=(0, 0, 0),
         pose=pose((1.0, 2.0, -0.5), 30.0, (0.137, -0.291, 0.053)), min_weight=float(MIN_WEIGHT)),
]
BY_NAME = {c["name"]: c for c in CASES}


def replica_of(case):
    import merge_replica as mr
    f = ck.config_fields(case["cfg"])
    return mr.merge(f, case["dst"][0], case["dst"][1], case["src"][0], case["src"][1], mode=case["mode"], voxel_offset=case["voxel_offset"],
                    pose=case["pose"], min_weight=case["min_weight"], max_weight=float(MAX_WEIGHT))
