#!/usr/bin/env python3
"""Record, as SHA-256 digests, what the REFERENCE's own C++ returned for the inputs of the tests that pin the
product against it on larger data (tests/test_oracle_vs_reference.py, tests/test_exact_gzip.py, and the
file-level GPU tests in tests/test_gpu_parity.py and tests/test_gpu_python_module.py).

Run where oracle/_ref/libspz_ref.so can be built (it needs the reference's sources):

    make -C oracle && python tests/golden/make_reference_digests.py

Writes tests/golden/reference_digests.json: for every case, a digest of the inputs (so that a changed input
generator shows up as such), digests of the reference's outputs (stream bytes, file bytes, decoded float32 bit
patterns; tests/conftest.py `digest`) and the few small values the tests read directly.  Inputs are rebuilt here
exactly as the tests build them; keep the two in step.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from conftest import FIELDS, digest, digest_cloud  # noqa: E402
from oracle.pyoracle import Reference  # noqa: E402
from spz_amd.synth import make_cloud_numpy  # noqa: E402

R = Reference()


def record_load(out, key, cloud, n):
    assert cloud["num_points"] == n, key
    out[f"{key}/num_points"] = int(cloud["num_points"])
    for k in FIELDS:
        out[f"{key}/{k}"] = digest(cloud[k])


def oracle_vs_reference(out):
    # test_random_clouds_all_coordinate_pairs
    n = 3001
    for deg in range(4):
        for frm in range(9):
            key = f"clouds/deg{deg}/from{frm}"
            c = make_cloud_numpy(n, deg, 500 + 10 * deg + frm)
            sr = R.pack(c, n, deg, True, frm)
            to = (frm * 5 + 3) % 9
            out[f"{key}/input"] = digest_cloud(c)
            out[f"{key}/pack"] = digest(sr)
            record_load(out, f"{key}/unpack_to{to}", R.unpack(sr, n, deg, to), n)
    # test_quaternion_helpers
    rng = np.random.default_rng(8)
    q = rng.standard_normal((20000, 4)).astype(np.float32)
    q[:2000] = np.round(q[:2000])
    q[np.all(q[:, :] == 0, axis=1)] = [0, 0, 0, 1]
    out["quats/input"] = digest(q)
    out["quats/pack_from6"] = digest(R.pack_quat(q.reshape(-1), 6))
    # test_gzip_container_bytes
    rng = np.random.default_rng(3)
    for size in (0, 1, 16, 8191, 8192, 8193, 300_000, 3_000_000):
        data = (rng.integers(0, 256, size, dtype=np.uint16) >> (size % 3 + 2)).astype(np.uint8)
        out[f"gzip/size{size}/input"] = digest(data)
        out[f"gzip/size{size}"] = digest(R.compress_gzipped(data))
    # test_half_to_float_all_values
    out["half_to_float"] = digest(np.array([R.half_to_float(h) for h in range(65536)], np.float32))
    # test_convert_coordinates
    n, deg = 777, 3
    c = make_cloud_numpy(n, deg, 9)
    out["convert/input"] = digest_cloud(c)
    for frm, to in ((4, 6), (6, 7), (1, 8), (0, 3), (5, 5)):
        b = R.convert_coordinates(c["positions"], c["rotations"], c["sh"], n, deg, frm, to)
        for y, nm in zip(b, ("positions", "rotations", "sh")):
            out[f"convert/from{frm}_to{to}/{nm}"] = digest(y)
    # test_parallel_gzip_is_read_by_the_reference: the reference's loadSpz of the product's parallel member
    import spz_amd.spz as spz
    n, deg = 40_000, 3
    c = make_cloud_numpy(n, deg, 99)
    stream = R.pack(c, n, deg, True, 6)
    par = spz._compress_gzipped_parallel(stream.tobytes(), 4)
    assert par == spz._compress_gzipped_parallel(stream.tobytes(), 4), "the parallel member is not reproducible"
    one = spz._compress_gzipped(stream.tobytes())
    out["parallel_gzip/input"] = digest_cloud(c)
    out["parallel_gzip/pack"] = digest(stream)
    out["parallel_gzip/member"] = digest(np.frombuffer(par, np.uint8))
    record_load(out, "parallel_gzip/load_parallel", R.load_spz(np.frombuffer(par, np.uint8), n, deg, 7), n)
    record_load(out, "parallel_gzip/load_single", R.load_spz(np.frombuffer(one, np.uint8), n, deg, 7), n)


def exact_gzip(out):
    # test_default_save_path_on_a_real_stream_equals_zlib_and_the_reference
    n = 300_000
    c = make_cloud_numpy(n, 3, 21)
    stream = R.pack(c, n, 3, False, 6)
    out["exact_gzip/input"] = digest_cloud(c)
    out["exact_gzip/pack"] = digest(stream)
    out["exact_gzip/gzip"] = digest(R.compress_gzipped(stream))


def file_level(out, tmp):
    # test_whole_file_of_a_large_cloud_equals_the_reference_file
    n, deg = 120_000, 3
    c = make_cloud_numpy(n, deg, 77)
    want = R.save_spz(c, n, deg, True, 6)
    out["whole_file/input"] = digest_cloud(c)
    out["whole_file/save"] = digest(want)
    record_load(out, "whole_file/load_to7", R.load_spz(want, n, deg, 7), n)
    # test_baseline_config1_ply_to_spz_60k
    n, deg = 60_000, 3
    c = make_cloud_numpy(n, deg, 60)
    want = R.save_spz(c, n, deg, False, 0)
    out["config1/input"] = digest_cloud(c)
    out["config1/save"] = digest(want)
    record_load(out, "config1/load_to0", R.load_spz(want, n, deg, 0), n)
    # test_cli_tools_round_trip
    n, deg = 4321, 2
    c = make_cloud_numpy(n, deg, 77)
    ply = os.path.join(tmp, "in.ply")
    assert R.save_ply(c, n, deg, 0, ply) == 0
    want = R.save_spz(c, n, deg, False, 0)
    back = R.load_spz(want, n, deg, 0)
    ref_ply = os.path.join(tmp, "ref_back.ply")
    assert R.save_ply(back, n, deg, 0, ref_ply) == 0
    p = back["positions"].reshape(-1, 3)
    out["cli/input"] = digest_cloud(c)
    out["cli/ply_in"] = digest(np.fromfile(ply, np.uint8))
    out["cli/save"] = digest(want)
    out["cli/ply_back"] = digest(np.fromfile(ref_ply, np.uint8))
    out["cli/info_lines"] = [f"  {a}: {lo:g} to {hi:g}" for a, lo, hi in zip("XYZ", p.min(0), p.max(0))]


def main():
    import tempfile
    out = {}
    oracle_vs_reference(out)
    exact_gzip(out)
    with tempfile.TemporaryDirectory() as tmp:
        file_level(out, tmp)
    with open(os.path.join(HERE, "reference_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"reference_digests.json: {len(out)} entries")


if __name__ == "__main__":
    main()
