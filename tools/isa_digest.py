#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 assembly of every source in gnode/build.py's SOURCES, run in the build container:
tools/isa_digest.py [extra flags] > digests.txt.  Each function's text between its label and .Lfunc_end is hashed with `;`
comments dropped and its block labels renumbered in order of appearance, together with the kernel's .amdhsa descriptor (LDS
size, register counts, scratch), so two builds compare with `diff`: a refactor of device code that prints the same lines
executes the same instructions with the same resources.  --split prints two digests per function, its instructions and its
descriptor, so that a changed argument list (.amdhsa_kernarg_size is in the descriptor) can be told from changed code."""
import hashlib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gn-ode-sir_amd"))
from gnode import build  # noqa: E402
SPLIT = "--split" in sys.argv
EXTRA = [a for a in sys.argv[1:] if a != "--split"]


def assembly(src):
    cmd = ["/opt/rocm/bin/hipcc", *build.FLAGS, *EXTRA, "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src}: hipcc failed\n{r.stderr}")
    return r.stdout


def digests(text):
    """(name, digest) per function: its instructions, plus its kernel descriptor (LDS, register counts, scratch) if it is
    a kernel; SPLIT: the two hashed apart, "instructions descriptor"."""
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
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
    if SPLIT:
        return [(n, sha(bodies[n]) + " " + sha(desc.get(n, []))) for n in order]
    return [(n, sha(bodies[n] + ["--"] + desc.get(n, []))) for n in order]


HIP_SOURCES = [s for s in build.SOURCES if s.endswith(".hip")]      # (the .cpp units are host code: no device assembly)
with ThreadPoolExecutor(max_workers=min(16, len(HIP_SOURCES))) as pool:
    for src, text in zip(HIP_SOURCES, pool.map(assembly, HIP_SOURCES)):
        for name, d in digests(text):
            print(f"{src} {name} {d}")
