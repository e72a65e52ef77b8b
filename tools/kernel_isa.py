"""tools/kernel_isa.py [--csrc DIR] [sources...] — one line per device function of each source: instructions and a hash of its instruction stream (no GPU).

Each source (default: the render stages' units) is compiled to gfx950 assembly with the library's own flags (`make -s print-flags`,
`--cuda-device-only -S`).  A function's stream is its instructions and labels in order, with comments and assembler directives dropped and
local labels renamed by order of first appearance — so two builds give the same hash exactly when the compiler emitted the same
instructions with the same registers, wherever the function stood in its file.  Moving code between units without changing it keeps every
hash; `--csrc DIR` reads the sources (and the Makefile's flags) of another checkout, to compare against."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["hr_frame.hip", "hr_raygen.hip", "hr_trace.hip", "hr_shade.hip"]


def assembly(csrc, src):
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "unit.s")
        subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", asm], check=True, capture_output=True, cwd=csrc)
        return open(asm).read().splitlines()


def functions(text):
    """[(mangled name, [normalised stream lines])] in file order"""
    out, name, body, labels = [], None, [], {}

    def local(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    for line in text:
        code = line.split(";")[0].rstrip()
        if not code.strip():
            continue
        if name is None:
            m = re.match(r"([A-Za-z_][\w$.]*):$", code)
            if m and not code.startswith(".L"):
                name, body, labels = m.group(1), [], {}
            continue
        if code.startswith(".Lfunc_end"):
            out.append((name, body))
            name = None
            continue
        if code.lstrip().startswith(".") and not re.match(r"\.L[\w$]+:$", code):
            continue  # an assembler directive
        body.append(re.sub(r"\.L[\w$]+", local, " ".join(code.split())))
    return out


def main():
    args = sys.argv[1:]
    csrc = os.path.join(ROOT, "heatray_amd", "csrc")
    if args[:1] == ["--csrc"]:
        csrc, args = os.path.abspath(args[1]), args[2:]
    srcs = args or DEFAULT
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1, 16)) as ex:
        texts = list(ex.map(lambda s: assembly(csrc, s), srcs))
    for src, text in zip(srcs, texts):
        fns = functions(text)
        names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in fns), capture_output=True, text=True).stdout.splitlines()
        for (_, body), name in zip(fns, names):
            n = sum(1 for l in body if not l.endswith(":"))
            print(f"{src:16s} {n:6d} {hashlib.sha256(chr(10).join(body).encode()).hexdigest()[:16]}  {name.split('(')[0]}")


if __name__ == "__main__":
    main()
