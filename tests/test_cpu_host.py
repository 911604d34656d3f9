"""-m "not gpu": host-side logic of the khronos::ActiveWindow mirror (no device needed)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
REF_CFG = os.path.join(ROOT, "tests", "golden", "uHumans2.yaml")  # the reference's khronos_ros/config/mapper/uHumans2.yaml, as a fixture

UHUMANS2_ACTIVE_WINDOW = """
# keys and values of khronos_ros/config/mapper/uHumans2.yaml:3-100 (shared anchors + active_window block)
shared_parameters:
  max_range: &max_range 5 # m
  temporal_window: &temporal_window 3 # s
  active_window_threads: &active_window_threads -1
active_window:
  type: "ActiveWindow"
  verbosity: 2
  min_output_separation: 0.4 # s
  frame_data_buffer:
    max_buffer_size: 300
    store_every_n_frames: 1
  volumetric_map:
    voxel_size: 0.1 # m
    truncation_distance: 0.2 # m (Usually 2-3x voxel size)
    voxels_per_side: 16
    with_semantics: true  # Enable semantic layer for object detection
  motion_detector:
    type: "FreeSpaceMotionDetector" # 'FreeSpaceMotionDetector'
    min_cluster_size: 500 # pixels
    min_separation_distance: 2 # voxels
    num_threads: *active_window_threads
    max_range: *max_range # m
  object_detector:
    type: "ConnectedSemantics"
    min_cluster_size: 50 # pixels
  tracker:
    verbosity: 0
    type: "MaxIouTracker"
  projective_integrator:
    num_threads: *active_window_threads
  tracking_integrator:
    temporal_window: *temporal_window
    num_threads: *active_window_threads
  object_extractor:
    type: MeshObjectExtractor
    min_object_volume: 0.005 # m^3
    max_object_volume: 10.0 # m^3
    only_extract_reconstructed_objects: true # used to be false
    object_reconstruction_resolution: -0.02
    projective_integrator:
      num_threads: 8
"""

EXPECT = {"voxel_size": 0.1, "truncation_distance": 0.2, "voxels_per_side": 16, "with_semantics": 1,
          "min_output_separation": 0.4, "motion_detector": "FreeSpaceMotionDetector", "md_min_cluster_size": 500,
          "md_min_separation_distance": 2, "md_max_range": 5, "temporal_window": 3, "object_extractor": "MeshObjectExtractor",
          "min_object_volume": 0.005, "max_buffer_size": 300, "object_detector": "ConnectedSemantics", "tracker": "MaxIouTracker",
          "only_extract_reconstructed_objects": 1, "object_reconstruction_resolution": -0.02}


def _parse(path):
    out = subprocess.run([SELFTEST, str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def test_host_selftest_known_answers(tmp_path):
    # (the selftest writes a stats.csv into $TMPDIR: a directory of this test's own)
    out = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=60, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0, out.stderr
    assert "host selftest ok" in out.stdout


def test_yaml_loader_reads_reference_keys(tmp_path):
    p = tmp_path / "aw.yaml"
    p.write_text(UHUMANS2_ACTIVE_WINDOW)
    got = _parse(p)
    for k, v in EXPECT.items():
        assert got[k] == (v if isinstance(v, str) else __import__("pytest").approx(v, rel=1e-6)), k


def test_yaml_loader_on_reference_file_when_present():
    # the reference's whole config file (tests/golden/uHumans2.yaml), not only the keys copied above
    got = _parse(REF_CFG)
    for k, v in EXPECT.items():
        assert got[k] == (v if isinstance(v, str) else __import__("pytest").approx(v, rel=1e-6)), k


def test_yaml_loader_reads_the_extractors_own_integrators_and_the_upstream_switches(tmp_path):
    """MeshObjectExtractor::Config nests its own projective_integrator / mesh_integrator blocks (mesh_object_extractor.cpp:63-64;
    uHumans2.yaml:99-100): they parse into the extractor's config, independent of the window's blocks of the same names.  The
    ASSUMPTIONS.md [A] switches parse by name and refuse unknown values."""
    text = ("active_window:\n  type: ActiveWindow\n"
            "  projective_integrator:\n    max_weight: 500\n    alloc_candidate: camera_offset\n    color_blend_weight: pre\n"
            "  mesh_integrator:\n    min_weight: 0.001\n    attr_source: containing\n    degenerate_eps: 1.0e-5\n"
            "  object_extractor:\n    type: MeshObjectExtractor\n    min_object_volume: 0.01\n"
            "    projective_integrator:\n      interpolation_method: nearest\n      max_weight: 40\n      use_weight_dropoff: false\n      num_threads: 8\n"
            "    mesh_integrator:\n      min_weight: 0.02\n      integrator_threads: 8\n")
    p = tmp_path / "aw.yaml"
    p.write_text(text)
    got = _parse(p)
    approx = __import__("pytest").approx
    assert got["alloc_candidate"] == "camera_offset" and got["color_blend_weight"] == "pre" and got["mesh_attr_source"] == "containing"
    assert got["mesh_degenerate_eps"] == approx(1e-5)
    assert got["object_interpolation_method"] == "nearest" and got["object_max_weight"] == approx(40.0) and got["object_use_weight_dropoff"] == 0
    assert got["object_mesh_min_weight"] == approx(0.02)
    assert got["object_color_blend_weight"] == "post" and got["object_mesh_attr_source"] == "nearest"  # (not inherited from the window's)
    for bad in ("    alloc_candidate: corner\n", "    color_blend_weight: during\n"):
        p.write_text("active_window:\n  projective_integrator:\n" + bad)
        out = subprocess.run([SELFTEST, str(p)], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0, bad


# ---- tracker plugins: C++ host restatement vs an independent Python restatement on random scenarios ----------
def _scenario(rng, n_frames, with_dynamic):
    """blobs of voxels drifting on a 0.2 m grid: some persist (static objects), one moves (dynamic), some flicker."""
    import numpy as np
    frames = []
    blobs = []
    for k in range(5):
        c = rng.integers(-10, 10, 3)
        ext = rng.integers(1, 4, 3)
        blobs.append(dict(center=c, ext=ext, cat=int(rng.integers(7, 10)), p_seen=float(rng.uniform(0.6, 1.0))))
    mover = np.array([0.0, 0.0, 2.0])
    for i in range(n_frames):
        stamp = 1_000_000_000 + i * 100_000_000
        sem, dyn = [], []
        next_id = 1
        for b in blobs:
            if rng.uniform() > b["p_seen"]:
                continue
            jitter = rng.integers(-1, 2, 3) if rng.uniform() < 0.3 else np.zeros(3, int)
            lo = b["center"] - b["ext"] + jitter
            hi = b["center"] + b["ext"] + jitter
            vox = {(int(x), int(y), int(z)) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)
                   if rng.uniform() < 0.9}
            if not vox:
                continue
            box = (np.array(lo, np.float32) * np.float32(0.2), (np.array(hi, np.float32) + 1) * np.float32(0.2))
            sem.append(dict(id=next_id, category=b["cat"], voxels=vox, box=box))
            next_id += 1
        rng.shuffle(sem)
        for k, c in enumerate(sem):
            c["id"] = k + 1
        if with_dynamic and i % 7 != 3:
            mover = mover + np.array([0.35, 0.1, 0.0])
            c0 = np.floor(mover / 0.2).astype(int)
            vox = {(int(c0[0] + x), int(c0[1] + y), int(c0[2] + z)) for x in range(-1, 2) for y in range(-1, 2) for z in range(-2, 3)}
            box = ((c0 - [1, 1, 2]).astype(np.float32) * np.float32(0.2), (c0 + [2, 2, 3]).astype(np.float32) * np.float32(0.2))
            dyn.append(dict(id=1, voxels=vox, box=box))
            if i % 5 == 0:  # the semantic detector sees the mover too
                sem.append(dict(id=len(sem) + 1, category=19, voxels=set(list(vox)[: len(vox) * 3 // 4]), box=box))
        frames.append((stamp, sem, dyn))
    return frames


def _encode(kind, cfg, frames):
    lines = ["C %s %s %s %r %r %r %r %r %d %r" % (kind, cfg["track_by"], cfg["association"], cfg["min_semantic_iou"], 0.0, cfg["min_cross_iou"],
                                                   cfg["max_dynamic_distance"], cfg["temporal_window"], cfg["min_num_observations"], cfg["voxel_size"])]

    def cl(tag, c, semantic):
        v = sorted(c["voxels"])
        head = "%s %d " % (tag, c["id"]) + ("%d " % c["category"] if semantic else "")
        return head + " ".join(repr(float(x)) for x in list(c["box"][0]) + list(c["box"][1])) + " %d " % len(v) + " ".join("%d %d %d" % t for t in v)
    for stamp, sem, dyn in frames:
        lines.append("F %d" % stamp)
        lines += [cl("S", c, True) for c in sem] + [cl("D", c, False) for c in dyn]
        lines.append("E")
    return "\n".join(lines) + "\n"


def _tracks_json(tr):
    return [dict(id=t.id, dyn=int(t.is_dynamic), active=int(t.is_active), conf=float(t.confidence), first=t.first_seen, last=t.last_seen,
                 cat=t.category if t.has_semantics else -1, n_obs=len(t.observations), obs=list(t.observations[-1]), n_vox=len(t.last_voxels),
                 centroid=[float(x) for x in t.last_centroid]) for t in tr.tracks]


def test_tracker_plugins_match_independent_restatement():
    import numpy as np
    import pytest
    import py_tracker
    cases = [
        ("maxiou", dict(track_by="voxels", association="assign_cluster", min_semantic_iou=0.25, min_cross_iou=0.1, max_dynamic_distance=1.0,
                        temporal_window=0.55, min_num_observations=4, voxel_size=0.2), True),
        ("maxiou", dict(track_by="voxels", association="assign_track", min_semantic_iou=0.25, min_cross_iou=0.1, max_dynamic_distance=0.5,
                        temporal_window=0.35, min_num_observations=15, voxel_size=0.2), True),
        ("maxiou", dict(track_by="bounding_box", association="assign_cluster", min_semantic_iou=0.3, min_cross_iou=0.2, max_dynamic_distance=1.0,
                        temporal_window=1.0, min_num_observations=3, voxel_size=0.2), True),
        ("external", dict(track_by="voxels", association="assign_cluster", min_semantic_iou=0.5, min_cross_iou=0.5, max_dynamic_distance=1.0,
                          temporal_window=0.45, min_num_observations=5, voxel_size=0.2), False),
    ]
    for seed, (kind, cfg, with_dyn) in enumerate(cases):
        rng = np.random.default_rng(100 + seed)
        frames = _scenario(rng, 40, with_dyn)
        out = subprocess.run([SELFTEST, "--tracker"], input=_encode(kind, cfg, frames), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        got = [json.loads(l) for l in out.stdout.strip().splitlines()]
        if kind == "external":
            ref = py_tracker.ExternalTracker(cfg["temporal_window"], cfg["min_num_observations"])
        else:
            ref = py_tracker.MaxIoUTracker(cfg["track_by"], cfg["association"], cfg["min_semantic_iou"], 0.0, cfg["min_cross_iou"],
                                           cfg["max_dynamic_distance"], cfg["temporal_window"], cfg["min_num_observations"], cfg["voxel_size"])
        assert len(got) == len(frames)
        n_tracks_max = 0
        for (stamp, sem, dyn), g in zip(frames, got):
            ref.process(stamp, sem, dyn)
            want = _tracks_json(ref)
            assert len(g) == len(want), (kind, stamp)
            for a, b in zip(g, want):
                for k in ("id", "dyn", "active", "first", "last", "cat", "n_obs", "obs"):
                    assert a[k] == b[k], (kind, stamp, k, a, b)
                assert a["conf"] == pytest.approx(b["conf"], rel=1e-6)
                if kind != "external" and cfg["track_by"] == "voxels":
                    assert a["n_vox"] == b["n_vox"]
                assert a["centroid"] == pytest.approx(b["centroid"], rel=1e-6, abs=1e-6)
            n_tracks_max = max(n_tracks_max, len(g))
        assert n_tracks_max >= 4
        if kind == "maxiou":
            assert any(t["dyn"] for t in got[-1]) and any(not t["active"] for t in got[-1])


def test_yaml_sequence_items_with_colons(tmp_path):
    """a block-sequence entry is a mapping only when its colon is followed by a space (or ends the line) and stands outside quotes
    (ADVICE r04): times, URLs and quoted text with ": " are scalar items; "- k: v" opens a mapping"""
    p = tmp_path / "items.yaml"
    p.write_text("items:\n  - 12:30:05\n  - http://host:8080/x\n  - 'quoted: text'\n  - plain\n  - name: a\n    value: 3\n  - key:\n")
    exe = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
    out = subprocess.run([exe, "--yaml-items", str(p)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[:4] == ["S 12:30:05", "S http://host:8080/x", "S quoted: text", "S plain"], lines
    assert lines[4] == "M name=a value=3" and lines[5].startswith("M key="), lines


def test_host_library_exports_the_sharded_tick_abi():
    """libkhronos_amd_host.so loads on a CPU-only box and exports every entry point include/khronos_amd_dist.h declares
    (the RCCL tick; no compute, no communicator is created here)."""
    import ctypes
    import re
    from khronos_amd import host_capi
    hdr = open(os.path.join(ROOT, "include", "khronos_amd_dist.h")).read()
    declared = set(re.findall(r"\b(kdist_[a-z_]+)\s*\(", hdr))
    assert declared == {"kdist_unique_id", "kdist_create", "kdist_destroy", "kdist_stream", "kdist_gather_frames", "kdist_tick",
                        "kdist_output", "kdist_last_exchange", "kdist_last_mesh_exchange", "kdist_tick_own", "kdist_profile", "kdist_profile_get"}
    lib = ctypes.CDLL(host_capi.HOST_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name in declared:
        assert hasattr(lib, name), name
    # the loader sets prototypes for all of them
    lib2 = host_capi.load_host_library()
    assert lib2.kdist_create.restype is ctypes.c_void_p


def test_integration_snippet_compiles(tmp_path):
    """The `ActiveWindowHip` translation unit INTEGRATION.md shows a Khronos maintainer (the reference-side binding of the
    C ABI: a hydra::ActiveWindowModule with the (config, output queue) constructor, protected spinOnce, factory
    registration) is compiled against the stand-in Hydra types, so the document cannot drift from the headers."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    m = re.search(r"<!-- snippet:active_window_hip:begin -->\s*```cpp\n(.*?)```\s*<!-- snippet:active_window_hip:end -->", text, re.S)
    assert m, "INTEGRATION.md lost its ActiveWindowHip snippet markers"
    src = tmp_path / "active_window_hip.cpp"
    # (one extra line instantiates the factory entry, so that the registration lambda and the constructor are compiled too)
    src.write_text(m.group(1) + "\nint main() { return hydra::ActiveWindowFactory::has(\"ActiveWindowHip\") ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(root, "include"),
                        "-I", os.path.join(root, "khronos_amd", "host"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_public_headers_are_plain_c():
    """the drop-in boundary is a C ABI: both public headers must compile as C99 on their own (no C++ types, no torch)"""
    import subprocess
    inc = os.path.join(ROOT, "include")
    for hdr in ("khronos_amd.h", "khronos_amd_dist.h"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", inc, os.path.join(inc, hdr)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_update_kernel_keeps_its_registers(tmp_path):
    """k_fuse sits at the vector-register limit (168 of 512 / 3 waves per SIMD).  A vector register spilled INSIDE its item loop is
    scratch traffic, i.e. vector memory the compiler cannot count: every partial wait of the software pipeline falls back to
    vmcnt(0) and the kernel loses a third of its speed (seen in round 4: 72 -> 95 us after one more value became live in the
    band dispatch).  The device code of the default instantiations must therefore compile without vector-register spills, and
    the item loop must still wait for its loads with a partial vmcnt."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    asm = tmp_path / "dev.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-Wno-unused-value", "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage", "-o", str(asm),
                        os.path.join(root, "khronos_amd", "csrc", "khronos_amd.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # -Rpass remarks: "Function Name: <mangled>" followed by that function's resource lines
    blocks = re.split(r"remark: Function Name: ", r.stderr)
    seen = 0
    for b in blocks[1:]:
        name = b.split()[0]
        # the exact- and relaxed-arithmetic instantiations of the 16^3 window map with 4 and 8 z ranges, reference switches
        if not re.match(r"_ZN3khr6k_fuseILi16ELi[48]ELb1ELb[01]ELi12EEE", name):
            continue
        seen += 1
        m = re.search(r"VGPRs Spill: (\d+)", b)
        assert m and int(m.group(1)) == 0, (name, m.group(0) if m else b[:400])
    assert seen == 4, seen
    text = asm.read_text()
    start = text.index("_ZN3khr6k_fuseILi16ELi4ELb1ELb1ELi12EEEvNS_8FuseArgsENS_8FuseListE:")
    body = text[start:text.index("s_endpgm", start)]
    assert "scratch_" not in body
    # the item loop = the outer loop (the inner ones are the band phase's chunks and the queue's spin wait)
    loop = body[body.index("=>This Loop Header: Depth=1"):]
    waits = [int(x) for x in re.findall(r"s_waitcnt vmcnt\((\d+)\)", "\n".join(loop.splitlines()[:4000]))]
    # phase 2 of an item waits for ITS loads while the next item's 16 loads and the previous item's stores stay in flight
    assert max(waits) >= 28 and sum(1 for w in waits if w >= 16) >= 12, waits
