"""Runs the reference's own code, compiled for the CPU (TEST INFRASTRUCTURE ONLY).

oracle/ref/build_ref.py (`make -C oracle ref`) builds two programs from the reference tree into
oracle/_ref/: ref_driver_gxx and ref_driver_clang.  This module writes a case file of plain arrays,
runs one of them and reads the arrays it wrote back (format: oracle/ref/ref_driver.cpp).  The CPU
tests tests/test_reference_parity.py and tools/make_reference_fixtures.py use it; no GPU test,
smoke() or bench.py does.

The two programs differ in one thing this project cares about: C++ leaves the evaluation order of
vec3(curand_uniform(s) - 0.5f, curand_uniform(s) - 0.5f, curand_uniform(s) - 0.5f) to the compiler;
clang++ draws x, y, z (the oracle's default), g++ draws z, y, x (orc.set_draw_order(True)).

The named switches, one per documented deviation of the oracle:
  powf          "mul" (default): powf(x, 5) as ((x*x)*(x*x))*x, what the oracle and the kernels do;
                "libm": libm's powf.
  camera_draws  "isolated" (default): the lens and time draws that camera::get_ray takes from
                randState[0] (main.cu:286) disturb pixel 0's stream only when pixel 0 itself renders;
                "shared": the reference untouched, pixels in launch order.  Either way pixel 0 is
                the one pixel a frame comparison leaves out.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "_ref")
DRIVERS = {"gxx": os.path.join(REF_DIR, "ref_driver_gxx"), "clang": os.path.join(REF_DIR, "ref_driver_clang")}
COMPILERS = ("clang", "gxx")
DRAW_ORDER_ZYX = {"clang": False, "gxx": True}   # the orc.set_draw_order() argument each program pins

OBJECT_DTYPE = np.dtype([("type", "<i4"), ("mat", "<i4"), ("v", "<f4", (9,))])
MATERIAL_DTYPE = np.dtype([("type", "<i4"), ("albedo", "<f4", (3,)), ("fuzz", "<f4"), ("ir", "<f4")])
HIT_DTYPE = np.dtype([("hit", "<i4"), ("obj", "<i4"), ("mat", "<i4"), ("front_face", "<i4"),
                      ("t", "<f4"), ("p", "<f4", (3,)), ("n", "<f4", (3,))])
NODE_DTYPE = np.dtype([("left", "<i4"), ("right", "<i4"), ("parent", "<i4"), ("objid", "<i4"),
                       ("bmin", "<f4", (3,)), ("bmax", "<f4", (3,))])
DIRECTIONS = {"forward": 0, "backward": 1, "left": 2, "right": 3, "up": 4, "down": 5}   # utils::directions


def available() -> bool:
    return all(os.access(p, os.X_OK) for p in DRIVERS.values())


def _write(path, arrays):
    with open(path, "wb") as f:
        f.write(b"PTRF" + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            data = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(data)) + data)


def _read(path):
    out = {}
    with open(path, "rb") as f:
        assert f.read(4) == b"PTRF"
        for _ in range(struct.unpack("<I", f.read(4))[0]):
            name = f.read(struct.unpack("<I", f.read(4))[0]).decode()
            out[name] = f.read(struct.unpack("<Q", f.read(8))[0])
    return out


def run(compiler: str, op: str, arrays: dict, powf: str = "mul", camera_draws: str = "isolated", timeout=600) -> dict:
    assert powf in ("mul", "libm") and camera_draws in ("isolated", "shared")
    with tempfile.TemporaryDirectory(prefix="ptref_") as d:
        src, dst = os.path.join(d, "in.ptrf"), os.path.join(d, "out.ptrf")
        _write(src, {"op": op.encode(), **arrays})
        p = subprocess.run([DRIVERS[compiler], src, dst, f"--powf={powf}", f"--camera-draws={camera_draws}"],
                           capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError(f"ref_driver_{compiler} {op}: exit {p.returncode}\n{p.stderr[-2000:]}")
        out = _read(dst)
    assert out["compiler"].decode() == compiler
    return out


def _objects(objects):
    return np.ascontiguousarray(objects, OBJECT_DTYPE)


def morton_keys(compiler, objects) -> np.ndarray:
    """computeMortonOnHost: the sorted 64-bit keys (code << 32 | object id)."""
    return np.frombuffer(run(compiler, "morton", {"objects": _objects(objects)})["keys"], np.uint64).copy()


def build_lbvh(compiler, objects):
    """buildBVH (generateLBVH + growBBox): (keys, nodes); the boxes are the reference's own,
    every internal one seeded with the origin."""
    out = run(compiler, "lbvh", {"objects": _objects(objects)})
    return np.frombuffer(out["keys"], np.uint64).copy(), np.frombuffer(out["nodes"], NODE_DTYPE).copy()


def trace(compiler, objects, rays, tmin=0.001, tmax=float("inf"), brute=False) -> np.ndarray:
    """hitBvh on the reference's own tree (or RenderManager::hit): closest-hit records.  `obj` is -1
    (hit_record has no object id); a miss has mat -1 and zeros elsewhere, like orc.trace."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = run(compiler, "trace", {"objects": _objects(objects), "rays": rays,
                                  "interval": np.array([tmin, tmax], np.float32),
                                  "brute": np.array([int(brute)], np.int32)})
    return np.frombuffer(out["hits"], HIT_DTYPE).copy()


def scatter(compiler, materials, case_mat, case_ray, case_hit, tapes, powf="mul"):
    """Material::scatter on cases (material index, incoming ray, hit record, tape of uniforms; the
    tape is followed by 0.5s like the oracle's): (ok, out_ray (k, 6), atten (k, 3), used)."""
    k = len(case_mat)
    tapes = np.ascontiguousarray(tapes, np.float32).reshape(k, -1)
    out = run(compiler, "scatter", {"materials": np.ascontiguousarray(materials, MATERIAL_DTYPE),
                                    "case_mat": np.ascontiguousarray(case_mat, np.int32),
                                    "case_ray": np.ascontiguousarray(case_ray, np.float32).reshape(k, 6),
                                    "case_hit": np.ascontiguousarray(case_hit, HIT_DTYPE),
                                    "tapes": tapes}, powf=powf)
    return (np.frombuffer(out["ok"], np.int32).copy(), np.frombuffer(out["out_ray"], np.float32).reshape(k, 6).copy(),
            np.frombuffer(out["atten"], np.float32).reshape(k, 3).copy(), np.frombuffer(out["used"], np.int32).copy())


def reflectance(compiler, cosine, ref_idx, powf="mul") -> np.ndarray:
    """rayphysics::reflectance(cosine[i], ref_idx[i]) (physical.h:20-25)."""
    out = run(compiler, "reflectance", {"cosine": np.ascontiguousarray(cosine, np.float32),
                                        "ref_idx": np.ascontiguousarray(ref_idx, np.float32)}, powf=powf)
    return np.frombuffer(out["r"], np.float32).copy()


def camera(compiler, args, move_dir, move_dt):
    """camera's constructor on args (k, 12) = from, at, vfov, aspect, aperture, focus, t0, t1, then
    processKeyboard(move_dir[i][j], move_dt[i][j]) in turn (a direction < 0 is no move):
    (cams (k, 25), moved (k, M, 25)) in the oracle's 25-float layout."""
    args = np.ascontiguousarray(args, np.float32).reshape(-1, 12)
    k = len(args)
    move_dir = np.ascontiguousarray(move_dir, np.int32).reshape(k, -1)
    move_dt = np.ascontiguousarray(move_dt, np.float32).reshape(k, -1)
    out = run(compiler, "camera", {"args": args, "move_dir": move_dir, "move_dt": move_dt})
    return (np.frombuffer(out["cams"], np.float32).reshape(k, 25).copy(),
            np.frombuffer(out["moved"], np.float32).reshape(k, move_dir.shape[1], 25).copy())


def render(compiler, objects, materials, camera_floats, width, height, spp, max_depth, seed, launches=1,
           powf="mul", camera_draws="isolated"):
    """initRandom(seed), then `launches` x render on the reference's own tree:
    (rgb (launches, w*h, 3) float32, states (launches, w*h, 6) uint32 after each launch)."""
    out = run(compiler, "render", {"objects": _objects(objects),
                                   "materials": np.ascontiguousarray(materials, MATERIAL_DTYPE),
                                   "camera": np.ascontiguousarray(camera_floats, np.float32).reshape(25),
                                   "params": np.array([width, height, spp, max_depth, launches, seed], np.int64)},
              powf=powf, camera_draws=camera_draws)
    n = width * height
    return (np.frombuffer(out["rgb"], np.float32).reshape(launches, n, 3).copy(),
            np.frombuffer(out["states"], np.uint32).reshape(launches, n, 6).copy())
