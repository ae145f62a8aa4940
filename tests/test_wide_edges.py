"""CPU test of the edge-form triangle records (host/pt_wide8.hpp edgeTriRecords).

The wide render kernels' LEAF step on a triangle-only scene reads records {v0, rank}{v1 - v0}{v2 -
v0} instead of the vertices: the two subtractions of every triangle test, done once per triangle.
tests/cpp/wide8_edges_check.cpp (test infrastructure, built here with g++) builds bunny_cornell's
wide tree exactly as libpt.so does, converts its records and compares every edge word with the fp32
subtraction of the vertex words, bit for bit; hand-made records cover edges that are denormal and
edges that cancel to +0 and -0.  The same program runs once more built with the address and
undefined-behaviour sanitizers (host code only).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "path-tracer-cuda-opengl_amd", "host")
SRC = os.path.join(ROOT, "tests", "cpp", "wide8_edges_check.cpp")


@pytest.fixture(scope="module")
def bunny_objects(pt, tmp_path_factory):
    p = pt.Preset("bunny_cornell", 32, 32)
    path = str(tmp_path_factory.mktemp("edges") / "objects.bin")
    p.objects.tofile(path)
    return path, len(p.objects)


def test_edge_records_equal_the_subtractions(bunny_objects, tmp_path):
    path, n = bunny_objects
    exe = str(tmp_path / "wide8_edges_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", HOST, SRC, os.path.join(HOST, "pt_wide8.cpp"), "-L", os.path.join(ROOT, "oracle"), "-loracle",
                    "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"{n} scene records"), r.stdout


def test_edge_records_under_sanitizers(bunny_objects, tmp_path):
    """A stand-alone program: the conversion, the host tree build and the oracle's LBVH compiled
    with -fsanitize=address,undefined; it must run clean."""
    path, n = bunny_objects
    exe = str(tmp_path / "wide8_edges_check_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                    "-I", HOST, "-I", os.path.join(ROOT, "oracle"), SRC, os.path.join(HOST, "pt_wide8.cpp"),
                    os.path.join(ROOT, "oracle", "pt_oracle.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=env)
    report = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.startswith(f"{n} scene records"), report[-4000:]
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert marker not in report, report[-4000:]
