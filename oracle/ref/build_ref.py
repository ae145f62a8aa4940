"""Build the reference's own code as two host programs: oracle/_ref/ref_driver_gxx and
oracle/_ref/ref_driver_clang (TEST INFRASTRUCTURE; `make -C oracle ref`).

The reference tree is read from $PT_REFERENCE_DIR (default /root/reference, where it lies on the
development machine).  When it is absent this script does nothing and succeeds: the tests that
run the harness then skip, and everything else -- every GPU test, smoke(), bench.py -- never
needs it.  Nothing of the reference is committed: its headers are copied at build time into
oracle/_ref/src/ (ignored by git), and the functions the driver needs from main.cu are cut out
of it there.

  1. utils/*.h and simulation/*.h  ->  oracle/_ref/src/ (one directory: render_manager.h includes
     "bvh.h" with quotes, so the includer's directory has to hold it);
  2. every `kernel<<<grid, block>>>(args)` in the copies becomes REF_LAUNCH(kernel, grid, block)(args),
     or REF_LAUNCH_SYNC(...) when the kernel's body calls __syncthreads (oracle/ref/shim.h);
  3. EXTRACT (below) are found in main.cu by signature and matching brace and written to
     oracle/_ref/src/main_extract.h; the rest of main.cu (GL, surfaces, scene builders) is not used;
  4. ref_driver.cpp + pt_oracle.cpp (for its XORWOW) are compiled with g++ and with the ROCm
     clang++, -O2 -ffp-contract=off, no fast-math.  g++ evaluates constructor arguments right to
     left and clang++ left to right, so the two programs pin the oracle's two draw orders.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.dirname(HERE)
OUT = os.path.join(ORACLE, "_ref")
SRC = os.path.join(OUT, "src")
REFERENCE = os.environ.get("PT_REFERENCE_DIR", "/root/reference")
EXTRACT = ("rayTracing", "initRandom", "render", "copyObjMatsToDevice", "copyBVHToDevice")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-pthread"]
DRIVERS = {"gxx": "ref_driver_gxx", "clang": "ref_driver_clang"}


def reference_present():
    try:
        return os.path.isfile(os.path.join(REFERENCE, "main.cu")) and os.path.isdir(os.path.join(REFERENCE, "utils"))
    except OSError:
        return False


def clangxx():
    cands = [os.environ.get("PT_REF_CLANGXX")]
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root:
            cands += [os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise SystemExit("build_ref: no ROCm clang++ found (set PT_REF_CLANGXX)")


def skip_code(text, i):
    """If text[i:] starts a comment, a string or a character literal, the index just past it; else i."""
    if text.startswith("//", i):
        j = text.find("\n", i)
        return len(text) if j < 0 else j
    if text.startswith("/*", i):
        j = text.find("*/", i + 2)
        return len(text) if j < 0 else j + 2
    if text[i] in "\"'":
        q, j = text[i], i + 1
        while j < len(text) and text[j] != q:
            j += 2 if text[j] == "\\" else 1
        return j + 1
    return i


def matching(text, start, open_ch, close_ch):
    """Index of the bracket that closes text[start] (an open_ch), skipping comments and literals."""
    assert text[start] == open_ch
    depth, i = 0, start
    while i < len(text):
        j = skip_code(text, i)
        if j != i:
            i = j
            continue
        if text[i] == open_ch:
            depth += 1
        elif text[i] == close_ch:
            depth -= 1
            if depth == 0:
                return i
        i += 1
    raise SystemExit(f"build_ref: unbalanced {open_ch}{close_ch} after offset {start}")


def find_function(text, name):
    """(start, end) of the definition `__device__|__global__ <type> name(...) {...}` in text, or None."""
    for m in re.finditer(r"__(?:device|global)__\s+[\w:]+\s+" + re.escape(name) + r"\s*\(", text):
        close = matching(text, m.end() - 1, "(", ")")
        k = close + 1
        while k < len(text) and text[k].isspace():
            k += 1
        if k < len(text) and text[k] == "{":   # a definition, not a declaration
            return m.start(), matching(text, k, "{", "}") + 1
    return None


def kernel_syncs(name, texts):
    for t in texts:
        span = find_function(t, name)
        if span:
            return "__syncthreads" in t[span[0]:span[1]]
    return False


def rewrite_launches(text, texts):
    def sub(m):
        macro = "REF_LAUNCH_SYNC" if kernel_syncs(m.group(1), texts) else "REF_LAUNCH"
        return f"{macro}({m.group(1)}, {m.group(2)})("
    return re.sub(r"(\w+)\s*<<<(.*?)>>>\s*\(", sub, text)


def newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def main():
    if not reference_present():
        print(f"build_ref: no reference tree at {REFERENCE}: nothing to build")
        return 0
    headers = sorted(glob.glob(os.path.join(REFERENCE, "utils", "*.h")) +
                     glob.glob(os.path.join(REFERENCE, "simulation", "*.h")))
    main_cu = os.path.join(REFERENCE, "main.cu")
    own = [os.path.join(HERE, f) for f in ("shim.h", "ref_driver.cpp", "build_ref.py")]
    own += glob.glob(os.path.join(HERE, "stubs", "*")) + [os.path.join(ORACLE, "pt_oracle.cpp"), os.path.join(ORACLE, "pt_oracle.h")]
    outs = [os.path.join(OUT, d) for d in DRIVERS.values()]
    if all(os.path.exists(o) for o in outs) and min(os.path.getmtime(o) for o in outs) > newest(headers + [main_cu] + own):
        print("build_ref: oracle/_ref is up to date")
        return 0

    shutil.rmtree(SRC, ignore_errors=True)
    os.makedirs(SRC)
    texts = {h: open(h, encoding="utf-8", errors="replace").read() for h in headers}
    main_text = open(main_cu, encoding="utf-8", errors="replace").read()
    everything = list(texts.values()) + [main_text]
    for h, t in texts.items():
        with open(os.path.join(SRC, os.path.basename(h)), "w", encoding="utf-8") as f:
            f.write(rewrite_launches(t, everything))
    parts = []
    for name in EXTRACT:
        span = find_function(main_text, name)
        if span is None:
            raise SystemExit(f"build_ref: {name} not found in {main_cu}")
        parts.append(main_text[span[0]:span[1]])
    with open(os.path.join(SRC, "main_extract.h"), "w", encoding="utf-8") as f:
        f.write("// cut out of the reference's main.cu at build time by oracle/ref/build_ref.py; never committed\n\n")
        f.write(rewrite_launches("\n\n".join(parts), everything) + "\n")

    common = FLAGS + ["-include", os.path.join(HERE, "shim.h"), "-I", SRC, "-I", os.path.join(HERE, "stubs"),
                      os.path.join(HERE, "ref_driver.cpp")]
    for tag, cxx in (("gxx", os.environ.get("PT_REF_GXX", "g++")), ("clang", clangxx())):
        out = os.path.join(OUT, DRIVERS[tag])
        xorwow = os.path.join(OUT, f"pt_oracle_{tag}.o")   # the shim is not forced onto the oracle's own text
        subprocess.run([cxx] + FLAGS + ["-c", os.path.join(ORACLE, "pt_oracle.cpp"), "-o", xorwow], check=True)
        # -w: the reference's own warnings (printf formats, sign compares) are not this project's to fix
        cmd = [cxx] + common + ["-w", xorwow, f"-DREF_COMPILER=\"{tag}\"", "-o", out + ".tmp"]
        subprocess.run(cmd, check=True)
        os.replace(out + ".tmp", out)
        print(f"build_ref: {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
