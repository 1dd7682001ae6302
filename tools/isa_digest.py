#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 assembly of every source in gnode/build.py's SOURCES, run in the build container:
tools/isa_digest.py [extra flags] > digests.txt.  Each function's text between its label and .Lfunc_end is hashed with `;`
comments dropped and its block labels renumbered in order of appearance, together with the kernel's .amdhsa descriptor (LDS
size, register counts, scratch), so two builds compare with `diff`: a refactor of device code that prints the same lines
executes the same instructions with the same resources."""
import hashlib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd"))
from gnode import build  # noqa: E402


def assembly(src):
    cmd = ["/opt/rocm/bin/hipcc", *build.FLAGS, *sys.argv[1:], "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src}: hipcc failed\n{r.stderr}")
    return r.stdout


def digests(text):
    """(name, digest) per function: its instructions, plus its kernel descriptor (LDS, register counts, scratch) if it is
    a kernel."""
    bodies, order, desc, name, labels = {}, [], {}, None, {}
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line) or re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name, labels = m.group(1), {}
            if line.lstrip().startswith(".amdhsa_kernel"):
                cur = desc.setdefault(name, [])
            else:
                cur = bodies.setdefault(name, [])
                order.append(name)
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end") or ".end_amdhsa_kernel" in line:
            name = None
            continue
        s = line.split(";")[0].strip()
        if s:
            cur.append(re.sub(r"\.LBB\d+_\d+", lambda b: labels.setdefault(b.group(0), f".LBB{len(labels)}"), s))
    return [(n, hashlib.sha256("\n".join(bodies[n] + ["--"] + desc.get(n, [])).encode()).hexdigest()[:16]) for n in order]


HIP_SOURCES = [s for s in build.SOURCES if s.endswith(".hip")]      # (the .cpp units are host code: no device assembly)
with ThreadPoolExecutor(max_workers=min(16, len(HIP_SOURCES))) as pool:
    for src, text in zip(HIP_SOURCES, pool.map(assembly, HIP_SOURCES)):
        for name, d in digests(text):
            print(f"{src} {name} {d}")
