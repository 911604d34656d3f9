"""Plain-numpy codec of the map checkpoint format (include/khronos_amd.h, ASSUMPTIONS.md A.11): needs no device and no library.

A checkpoint is one byte stream: a 256-byte header, then one section per layer, each on a 64-byte boundary, blocks in the
lexicographic (x, y, z) order of their indices, voxels in linear order.  Layers of `pack` / `unpack` (n blocks, nv = vps^3):
    distance, weight   (n, nv) float32            color          (n, nv, 4) uint8
    last_observed, last_occupied (n, nv) uint64   (with_tracking)
    flags              (n, nv) uint8  KHR_VOX_* bits
    sem_label          (n, nv) uint32             (with_semantics)
    block_flags        (n,)  uint8   KHR_BLK_* bits
    likelihoods        (n, nv, num_labels) float32, voxel-major (with_semantics)
"""
import struct

import numpy as np

MAGIC, VERSION, HEADER_BYTES = 0x4D52484B, 1, 256
SECTIONS = ("indices", "distance", "weight", "color", "last_observed", "last_occupied", "flags", "sem_label", "block_flags",
            "likelihoods")
CONFIG_FIELDS = ("voxel_size", "voxels_per_side", "truncation_distance", "with_semantics", "with_tracking", "num_labels",
                 "semantic_mode")
_HEADER = struct.Struct("<IIfifiiiiIQQ10Q")
_DTYPES = {"indices": np.int32, "distance": np.float32, "weight": np.float32, "color": np.uint8, "last_observed": np.uint64,
           "last_occupied": np.uint64, "flags": np.uint8, "sem_label": np.uint32, "block_flags": np.uint8,
           "likelihoods": np.float32}


class CheckpointError(ValueError):
    pass


def config_fields(cfg):
    """the header's configuration fields from a khr_config-like object or a dict, normalised as the library stores them"""
    get = cfg.get if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    sem = 1 if get("with_semantics") else 0
    return {"voxel_size": float(np.float32(get("voxel_size"))), "voxels_per_side": int(get("voxels_per_side")),
            "truncation_distance": float(np.float32(get("truncation_distance"))), "with_semantics": sem,
            "with_tracking": 1 if get("with_tracking") else 0, "num_labels": int(get("num_labels")) if sem else 0,
            "semantic_mode": int(get("semantic_mode") or 0) if sem else 0}


def _shapes(f, n):
    """per section: (element shape of the whole section, bytes per block), None for a layer the configuration lacks"""
    nv = f["voxels_per_side"] ** 3
    trk, sem, K = f["with_tracking"], f["with_semantics"], f["num_labels"]
    return {"indices": ((n, 3), 12), "distance": ((n, nv), 4 * nv), "weight": ((n, nv), 4 * nv), "color": ((n, nv, 4), 4 * nv),
            "last_observed": ((n, nv), 8 * nv) if trk else None, "last_occupied": ((n, nv), 8 * nv) if trk else None,
            "flags": ((n, nv), nv), "sem_label": ((n, nv), 4 * nv) if sem else None, "block_flags": ((n,), 1),
            "likelihoods": ((n, nv, K), 4 * nv * K) if sem else None}


def _offsets(f, n):
    at, off = HEADER_BYTES, {}
    for name in SECTIONS:
        sh = _shapes(f, n)[name]
        off[name] = at if sh else 0
        at += ((sh[1] * n if sh else 0) + 63) // 64 * 64
    return off, at


def pack(config, indices, layers, sort=True):
    """bytes of the checkpoint of the blocks `indices` (n, 3) with the layers above; `config`: the CONFIG_FIELDS (dict or
    khr_config).  sort=True orders the blocks as the format wants them; sort=False writes them as given."""
    f = config_fields(config)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    n = len(idx)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0])) if sort else np.arange(n)
    off, total = _offsets(f, n)
    out = np.zeros(total, np.uint8)
    out[:_HEADER.size] = np.frombuffer(_HEADER.pack(MAGIC, VERSION, f["voxel_size"], f["voxels_per_side"], f["truncation_distance"],
                                                    f["with_semantics"], f["with_tracking"], f["num_labels"], f["semantic_mode"],
                                                    HEADER_BYTES, n, total, *[off[s] for s in SECTIONS]), np.uint8)
    shapes = _shapes(f, n)
    for name in SECTIONS:
        if shapes[name] is None:
            continue
        a = idx if name == "indices" else np.asarray(layers[name])
        a = np.ascontiguousarray(a, _DTYPES[name]).reshape(shapes[name][0])[order]
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        out[off[name]: off[name] + raw.size] = raw
    return out.tobytes()


def read_header(buf):
    """header dict of a stream, validated as khr_checkpoint_inspect validates it"""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    if a.size < HEADER_BYTES:
        raise CheckpointError("truncated buffer (%d bytes, the header alone has %d)" % (a.size, HEADER_BYTES))
    v = _HEADER.unpack(a[:_HEADER.size].tobytes())
    h = dict(zip(("magic", "version") + CONFIG_FIELDS + ("header_bytes", "num_blocks", "total_bytes"), v[:12]))
    h["offset"] = dict(zip(SECTIONS, v[12:]))
    if h["magic"] != MAGIC:
        raise CheckpointError("bad magic 0x%08x" % h["magic"])
    if h["version"] != VERSION:
        raise CheckpointError("unknown format version %d" % h["version"])
    if h["header_bytes"] != HEADER_BYTES or h["voxels_per_side"] not in (8, 16):
        raise CheckpointError("bad header")
    off, total = _offsets(h, h["num_blocks"])
    if off != h["offset"] or total != h["total_bytes"]:
        raise CheckpointError("section offsets are not the canonical ones")
    if a.size < total:
        raise CheckpointError("truncated buffer (%d bytes, the header claims %d)" % (a.size, total))
    return h


def unpack(buf):
    """(header dict, indices (n, 3) int32, layers dict) of a stream; the arrays are copies"""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1).view(np.uint8)
    h = read_header(a)
    n = h["num_blocks"]
    layers = {}
    for name, sh in _shapes(h, n).items():
        if sh is None:
            continue
        raw = a[h["offset"][name]: h["offset"][name] + sh[1] * n]
        layers[name] = raw.copy().view(_DTYPES[name]).reshape(sh[0])
    return h, layers.pop("indices"), layers


def pack_blocks(config, indices, get_block, sort=True):
    """pack() from per-block dicts as FusionContext.download_block / OracleMap.get_block return them (likelihoods [k][voxel])"""
    f = config_fields(config)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    blocks = [get_block(i) for i in idx]
    names = [s for s, sh in _shapes(f, len(idx)).items() if sh is not None and s not in ("indices", "likelihoods")]
    shapes = _shapes(f, len(idx))
    layers = {s: (np.stack([np.asarray(b[s]) for b in blocks]) if blocks else np.zeros(shapes[s][0], _DTYPES[s])) for s in names}
    if f["with_semantics"]:
        layers["likelihoods"] = (np.stack([np.asarray(b["likelihoods"], np.float32).T for b in blocks]) if blocks
                                 else np.zeros(shapes["likelihoods"][0], np.float32))
    return pack(f, idx, layers, sort=sort)


def block_view(layers, i):
    """block i of unpacked layers in the shape of download_block's dict (likelihoods [k][voxel])"""
    b = {k: v[i] for k, v in layers.items() if k != "likelihoods"}
    b["block_flags"] = int(layers["block_flags"][i])
    if "likelihoods" in layers:
        b["likelihoods"] = np.ascontiguousarray(layers["likelihoods"][i].T)
    return b
