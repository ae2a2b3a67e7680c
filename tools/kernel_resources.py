#!/usr/bin/env python3
"""Per-kernel register, spill, scratch, LDS and occupancy numbers of the device code, as the compiler reports them.

    python tools/kernel_resources.py [--json] [--filter SUBSTR] [-D...]       # a table (or JSON) on stdout

The device code is compiled once (-Rpass-analysis=kernel-resource-usage, device side only, nothing is written); the
report is cached by a hash of the sources and flags next to the built library (kmergutsjava_amd/.kernel_resources.json,
git-ignored), so that the ~20 s compile is paid once per source state.  Resource numbers only: no instruction is looked at.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
CACHE = os.path.join(ROOT, "kmergutsjava_amd", ".kernel_resources.json")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function"]

FIELDS = {                                  # the remark's label -> our key
    "TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
    "LDS Size [bytes/block]": "lds",
}


def hipcc() -> str | None:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _sources() -> list[str]:
    return [os.path.join(CSRC, "kmerguts_hip.hip")] + sorted(
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")) + [os.path.join(ROOT, "include", "kmerguts_hip.h")]


def _digest(extra: list[str]) -> str:
    h = hashlib.sha256()
    for s in _sources():
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS + extra).encode())
    return h.hexdigest()


def _demangle(names: list[str]) -> list[str]:
    filt = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(filt):
        filt = shutil.which("c++filt")
    if not filt:
        return names
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return out if len(out) == len(names) else names


def _short(demangled: str) -> str:
    """'void kg::part_scatter_kernel<false>(unsigned char const*, ...)' -> 'part_scatter_kernel<false>'"""
    s = demangled
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):                       # cut at the '(' of the parameter list (outside <>)
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            s = s[:i]
            break
    s = s.replace("kg::", "")
    return re.sub(r"\((\w+)\)(\d+)", r"\2", s).replace(", ", ",")      # (kg::Mode)1 -> 1


def parse(report: str) -> dict[str, dict[str, int]]:
    res: dict[str, dict[str, int]] = {}
    mangled: list[str] = []
    cur = None
    for line in report.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            if cur not in res:
                res[cur] = {}
                mangled.append(cur)
            continue
        m = re.search(r"remark: +([A-Za-z][^:]*): (\S+)", line)
        if m and cur and m.group(1).strip() in FIELDS:
            v = m.group(2)
            res[cur][FIELDS[m.group(1).strip()]] = int(v) if v.lstrip("-").isdigit() else 0
    names = [_short(d) for d in _demangle(mangled)]
    return {n: res[k] for n, k in zip(names, mangled)}


def resources(extra: list[str] | None = None, use_cache: bool = True) -> dict[str, dict[str, int]]:
    """{kernel: {sgprs, sgpr_spills, vgprs, vgpr_spills, agprs, scratch, lds, occupancy}}; raises without hipcc."""
    extra = list(extra or [])
    key = _digest(extra)
    if use_cache and os.path.exists(CACHE):
        try:
            with open(CACHE) as f:
                c = json.load(f)
            if c.get("key") == key:
                return c["kernels"]
        except (OSError, ValueError, KeyError):
            pass
    cc = hipcc()
    if not cc:
        raise RuntimeError("hipcc not found")
    cmd = [cc, *FLAGS, *extra, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, _sources()[0]]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError("hipcc failed:\n" + p.stderr[-4000:])
    kernels = parse(p.stderr)
    if not kernels:
        raise RuntimeError("the compiler printed no kernel-resource-usage remarks")
    if use_cache:
        try:
            tmp = CACHE + ".%d" % os.getpid()
            with open(tmp, "w") as f:
                json.dump({"key": key, "kernels": kernels}, f)
            os.replace(tmp, CACHE)
        except OSError:
            pass
    return kernels


def main(argv: list[str]) -> int:
    extra = [a for a in argv if a.startswith("-D")]
    filt = argv[argv.index("--filter") + 1] if "--filter" in argv else ""
    ks = resources(extra, use_cache="--no-cache" not in argv)
    ks = {k: v for k, v in ks.items() if filt in k}
    if "--json" in argv:
        print(json.dumps(ks, indent=1, sort_keys=True))
        return 0
    cols = ["sgprs", "sgpr_spills", "vgprs", "vgpr_spills", "scratch", "lds", "occupancy"]
    w = max(len(k) for k in ks) if ks else 6
    print("%-*s %s" % (w, "kernel", " ".join("%11s" % c for c in cols)))
    for k in sorted(ks):
        print("%-*s %s" % (w, k, " ".join("%11d" % ks[k].get(c, 0) for c in cols)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
