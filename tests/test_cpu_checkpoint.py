"""The map checkpoint format without a device: the numpy codec (khronos_amd/checkpoint.py) round-trips, and the library's header
inspection (khr_checkpoint_inspect, no context, no device) agrees with it and refuses what is not a checkpoint."""
import numpy as np
import pytest

from khronos_amd import checkpoint as ck
from khronos_amd.capi import KHR_EINVAL, checkpoint_inspect, load_library

LAYER_DTYPES = {"distance": np.float32, "weight": np.float32, "color": np.uint8, "last_observed": np.uint64, "last_occupied": np.uint64,
                "flags": np.uint8, "sem_label": np.uint32, "block_flags": np.uint8, "likelihoods": np.float32}


def random_map(rng, n, vps, sem, trk, K=5):
    nv = vps ** 3
    cfg = dict(voxel_size=0.07, voxels_per_side=vps, truncation_distance=0.21, with_semantics=sem, with_tracking=trk, num_labels=K,
               semantic_mode=0)
    idx = np.unique(rng.integers(-40, 40, (4 * n + 4, 3)), axis=0)
    idx = idx[rng.permutation(len(idx))][:n].astype(np.int32)
    layers = {"distance": rng.standard_normal((n, nv)).astype(np.float32), "weight": rng.random((n, nv)).astype(np.float32),
              "color": rng.integers(0, 256, (n, nv, 4)).astype(np.uint8), "flags": rng.integers(0, 16, (n, nv)).astype(np.uint8),
              "block_flags": rng.integers(0, 16, n).astype(np.uint8)}
    if trk:
        layers["last_observed"] = rng.integers(0, 2 ** 63, (n, nv)).astype(np.uint64)
        layers["last_occupied"] = rng.integers(0, 2 ** 63, (n, nv)).astype(np.uint64)
    if sem:
        layers["sem_label"] = rng.integers(0, K, (n, nv)).astype(np.uint32)
        layers["likelihoods"] = rng.standard_normal((n, nv, K)).astype(np.float32)
    return cfg, idx, layers


@pytest.mark.parametrize("vps", [16, 8])
@pytest.mark.parametrize("sem,trk", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_codec_round_trip(vps, sem, trk):
    rng = np.random.default_rng(vps * 10 + sem * 2 + trk)
    cfg, idx, layers = random_map(rng, 7, vps, sem, trk)
    blob = ck.pack(cfg, idx, layers)
    h, idx2, layers2 = ck.unpack(blob)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    assert np.array_equal(idx2, idx[order]) and idx2.dtype == np.int32
    assert h["num_blocks"] == 7 and h["total_bytes"] == len(blob)
    assert set(layers2) == set(layers), "layers the configuration does not have are absent from the stream"
    for k, v in layers.items():
        assert layers2[k].dtype == LAYER_DTYPES[k] and layers2[k].tobytes() == v[order].tobytes(), k
    for k in ("last_observed", "last_occupied"):
        assert (h["offset"][k] != 0) == bool(trk)
    for k in ("sem_label", "likelihoods"):
        assert (h["offset"][k] != 0) == bool(sem)
    assert h["num_labels"] == (5 if sem else 0)
    # packing the decoded stream again gives the same bytes (the stream is a function of the values alone)
    assert ck.pack(h, idx2, layers2) == blob
    # an empty map is a valid stream too
    e = ck.pack(cfg, np.zeros((0, 3), np.int32), {k: v[:0] for k, v in layers.items()})
    assert ck.unpack(e)[0]["num_blocks"] == 0 and len(e) == ck.HEADER_BYTES


@pytest.mark.parametrize("vps,sem,trk", [(16, 1, 1), (8, 0, 1), (8, 1, 0)])
def test_inspect_agrees_with_codec(vps, sem, trk):
    load_library()
    cfg, idx, layers = random_map(np.random.default_rng(3), 5, vps, sem, trk)
    blob = ck.pack(cfg, idx, layers)
    rc, h = checkpoint_inspect(blob)
    assert rc == 0
    mine = ck.read_header(blob)
    for k in ("magic", "version", "voxels_per_side", "with_semantics", "with_tracking", "num_labels", "semantic_mode", "header_bytes",
              "num_blocks", "total_bytes"):
        assert h[k] == mine[k], k
    assert np.float32(h["voxel_size"]) == np.float32(0.07) and np.float32(h["truncation_distance"]) == np.float32(0.21)
    assert h["offset"] == mine["offset"]
    assert h["magic"] == ck.MAGIC and h["version"] == ck.VERSION


def test_inspect_refuses_what_is_not_a_checkpoint():
    lib = load_library()
    cfg, idx, layers = random_map(np.random.default_rng(4), 3, 8, 1, 1)
    blob = bytearray(ck.pack(cfg, idx, layers))

    def err(b):
        rc, h = checkpoint_inspect(bytes(b))
        assert h is None
        return rc, lib.khr_last_error().decode()

    bad = bytearray(blob)
    bad[0] ^= 0xFF
    rc, text = err(bad)
    assert rc == KHR_EINVAL and "magic" in text
    bad = bytearray(blob)
    bad[4] = 2
    rc, text = err(bad)
    assert rc == KHR_EINVAL and "version" in text
    rc, text = err(blob[:-1])
    assert rc == KHR_EINVAL and "truncated" in text
    rc, text = err(blob[:100])
    assert rc == KHR_EINVAL and "truncated" in text
    for b in (bad, blob[:-1]):
        with pytest.raises(ck.CheckpointError):
            ck.read_header(bytes(b))
    assert checkpoint_inspect(bytes(blob))[0] == 0
