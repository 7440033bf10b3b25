#!/usr/bin/env python3
"""Which kernel instantiations of libmaxk_hip.so does the small GPU suite launch?

    symbols   the kernels of the gfx950 code objects inside the built library (names only: the
              offload bundles of the .hip_fatbin section are cut out, llvm-readelf --symbols
              lists each code object's `<kernel>.kd` descriptors, c++filt demangles them);
              needs no GPU
    trace     each small GPU test file once under `rocprofv3 --kernel-trace` (no counters, no
              other tracing, the program after `--`), one file per run, each under its own
              timeout; the mangled kernel names of every dispatch go to a JSON file.  A run
              that ends on a fault, an abort or its time limit stops the sequence.
    report    symbols x traces -> <out>.md and <out>.json: every instantiation with the test
              files that launch it, or its state from tests/variant_cases.py (the case that
              selects it, "wide, needs N bytes", "not launchable: rule ...") or "unreached"

    python tools/variant_reach.py trace --out build/reach/trace.json
    python tools/variant_reach.py report --trace build/reach/trace.json \
        --out profiles/r08/variant_reach/before

The tool is not a test and no test calls it.  test_fullsize_gpu, test_dist_gpu and
test_bench_gpu are left out of `trace` (not small; they spawn ranks); `trace --fullsize` adds
one traced run of test_fullsize_gpu, recorded apart from the small files.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "spgemm-prunning_amd", "lib", "libmaxk_hip.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NOT_SMALL = ("test_fullsize_gpu.py", "test_dist_gpu.py", "test_bench_gpu.py")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
STOP_CODES = (124, 137, 134, 139, -6, -11)  # time limit, abort, segmentation fault
LIBRARY_PREFIXES = ("rocprim::",)


def _tool(name):
    for p in (os.path.join(ROCM, "lib", "llvm", "bin", name), os.path.join(ROCM, "bin", name)):
        if os.path.exists(p):
            return p
    return shutil.which(name) or name


# ------------------------------------------------------------------------------- symbols
def code_objects(lib):
    """The gfx950 code objects of every offload bundle in the library, as bytes."""
    data = open(lib, "rb").read()
    out, at = [], data.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, at + len(MAGIC))
    if not out:
        raise SystemExit(f"{lib}: no gfx950 code object (compressed bundles are not read)")
    return out


def demangle(names):
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True,
                       text=True, check=True)
    return r.stdout.splitlines()


def short_name(demangled):
    """`void maxk::(anonymous namespace)::f<1, 2>(args)` -> `f<1, 2>`."""
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"^void ", "", s)
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.replace("maxk::", "")


def kernel_symbols(lib=LIB):
    """{mangled: short demangled name} of every kernel in the library."""
    mangled = set()
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"co{i}.elf")
            with open(path, "wb") as f:
                f.write(co)
            txt = subprocess.run([_tool("llvm-readelf"), "--symbols", "-W", path],
                                 capture_output=True, text=True, check=True).stdout
            for line in txt.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
                    mangled.add(f[7][:-3])
    mangled = sorted(mangled)
    return dict(zip(mangled, (short_name(d) for d in demangle(mangled))))


# ------------------------------------------------------------------------------- trace
def small_gpu_files():
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        if os.path.basename(path) in NOT_SMALL:
            continue
        if "pytest.mark.gpu" in open(path).read():
            out.append(os.path.basename(path))
    return out


def trace_file(name, tmp, limit):
    """One pytest file under rocprofv3 --kernel-trace; returns (exit code, kernel names)."""
    d = os.path.join(tmp, name)
    cmd = ["timeout", "-k", "10", str(limit), _tool("rocprofv3"), "--kernel-trace",
           "--mangled-kernels", "-f", "csv", "-d", d, "--",
           sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join("tests", name)]
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.run(cmd, cwd=ROOT).returncode
    names = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                n = row["Kernel_Name"]
                n = n[:-3] if n.endswith(".kd") else n
                names[n] = names.get(n, 0) + 1
    shutil.rmtree(d, ignore_errors=True)
    return rc, names


def cmd_trace(a):
    files = a.files or small_gpu_files()
    if a.fullsize:
        files = files + ["test_fullsize_gpu.py"]
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name in files:
            rc, names = trace_file(name, tmp, a.limit)
            result[name] = {"rc": rc, "dispatches": names}
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1, sort_keys=True)
            print(f"{name}: rc {rc}, {len(names)} distinct kernels, "
                  f"{sum(names.values())} dispatches", flush=True)
            if rc in STOP_CODES:
                print(f"{name} ended with {rc}: nothing more is started", flush=True)
                return 1
    return 0


# ------------------------------------------------------------------------------- report
def annotations():
    """(cases by kernel, wide, not launchable) from tests/variant_cases.py, empty before it exists."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import variant_cases as vc
    except ImportError:
        return {}, {}, {}
    by_kernel = {}
    for c in vc.CASES:
        for kern in c.kernels:
            by_kernel.setdefault(kern, []).append(c.id)
    return by_kernel, dict(vc.WIDE), dict(vc.NOT_LAUNCHABLE)


def _match(table, name):
    for pat, v in table.items():
        if re.fullmatch(pat, name):
            return v
    return None


def cmd_report(a):
    symbols = kernel_symbols(a.lib)
    traces = {}
    for path in a.trace:
        traces.update(json.load(open(path)))
    by_kernel, wide, dead = annotations() if a.annotate else ({}, {}, {})
    full = traces.get("test_fullsize_gpu.py")
    rows, library = {}, {}
    for mangled, name in symbols.items():
        small = sorted(f for f, t in traces.items()
                       if f not in NOT_SMALL and mangled in t["dispatches"])
        if name.startswith(LIBRARY_PREFIXES):
            # a device library's own kernels (rocprim's sort and scan behind the plan builders):
            # its dispatch picks among them, not a launch site of this project
            fam = library.setdefault(name.split("<")[0], {"instantiations": 0, "reached": 0})
            fam["instantiations"] += 1
            fam["reached"] += bool(small)
            continue
        if small:
            state = "reached"
        elif _match(dead, name) is not None:
            state = "not launchable: " + _match(dead, name)
        elif _match(wide, name) is not None:
            state = f"wide, needs {_match(wide, name)} bytes"
        else:
            state = "unreached"
        rows[name] = {"mangled": mangled, "files": small, "state": state,
                      "fullsize": ("not traced" if full is None else
                                   "reached" if mangled in full["dispatches"] else "unreached"),
                      "cases": by_kernel.get(name, [])}
    counts = {}
    for r in rows.values():
        key = r["state"].split(":")[0].split(",")[0]
        counts[key] = counts.get(key, 0) + 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump({"counts": counts, "files": {k: v["rc"] for k, v in traces.items()},
                   "instantiations": rows, "library_kernels": library}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    with open(a.out + ".md", "w") as f:
        f.write("# Kernel instantiations of libmaxk_hip.so and the small GPU tests that launch them\n\n")
        f.write("Written by `tools/variant_reach.py report`: kernel names from the gfx950 code "
                "objects of the built library, launches from `rocprofv3 --kernel-trace` of one "
                "test file per run.\n\n")
        f.write("Traced files (pytest exit code): " +
                ", ".join(f"{k[:-3]} ({v['rc']})" for k, v in sorted(traces.items())) + "\n\n")
        f.write("Counts: " + ", ".join(f"{k} {v}" for k, v in sorted(counts.items())) +
                f"; {len(rows)} instantiations\n\n")
        only_full = sorted(n for n, r in rows.items()
                           if not r["files"] and r["fullsize"] == "reached")
        f.write("Launched by no small test file but by the full-size run: " +
                (", ".join(f"`{n}`" for n in only_full) if only_full else
                 "none" if full is not None else "not traced") + "\n\n")
        f.write("| instantiation | state | small test files; case of test_variants_gpu | full-size run |\n"
                "|---|---|---|---|\n")
        for name in sorted(rows, key=lambda n: (rows[n]["state"] == "reached", n)):
            r = rows[name]
            where = ", ".join(x[5:-3] for x in r["files"])
            if r["cases"]:
                where += ("; " if where else "") + "case " + ", ".join(r["cases"])
            f.write(f"| `{name}` | {r['state']} | {where} | {r['fullsize']} |\n")
        f.write("\nKernels of device libraries linked into the code objects (their own dispatch "
                "selects among them):\n\n| kernel | instantiations | reached |\n|---|---|---|\n")
        for fam in sorted(library):
            f.write(f"| `{fam}` | {library[fam]['instantiations']} | {library[fam]['reached']} |\n")
    print(f"{a.out}.md: {counts}")
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("symbols")
    s.add_argument("--lib", default=LIB)
    t = sub.add_parser("trace")
    t.add_argument("--out", required=True, help="JSON of the traces (extended when it exists)")
    t.add_argument("--files", nargs="*", help="test files (default: every small GPU file)")
    t.add_argument("--fullsize", action="store_true")
    t.add_argument("--limit", type=int, default=420, help="seconds per file")
    r = sub.add_parser("report")
    r.add_argument("--lib", default=LIB)
    r.add_argument("--trace", nargs="+", required=True)
    r.add_argument("--out", required=True, help="path prefix of the .md and .json")
    r.add_argument("--no-annotate", dest="annotate", action="store_false",
                   help="leave tests/variant_cases.py out (the map before the cases)")
    a = p.parse_args()
    if a.cmd == "symbols":
        for name in sorted(kernel_symbols(a.lib).values()):
            print(name)
        return 0
    return cmd_trace(a) if a.cmd == "trace" else cmd_report(a)


if __name__ == "__main__":
    sys.exit(main())
