"""Compile the reference's own sources for the CPU: oracle/_ref/libref.so.

TEST INFRASTRUCTURE ONLY.  The reference tree (RT_REFERENCE_DIR, default
/root/reference) is read, never copied into the repository: its sources are
written to oracle/_ref/src/ (git-ignored) with two rewrites, both generic
patterns that name no identifier of the reference:
  - the kernel-launch chevrons, `k <<< g, b >>> (` -> `REF_LAUNCH(k, g, b)(`;
  - `template<>` in front of a member of a class-template specialization that
    is defined without it at file scope (`R C<A>::f(` -> `template<> R C<A>::f(`):
    MSVC accepts the omission, clang has no flag that does.
They compile as C++ against the stand-in headers of oracle/ref_shim/ (CUDA words defined away, a launch is a
loop), together with oracle/ref_harness.cpp, a C ABI over the reference's
classes.  oracle/_ref.py binds the library.

Flags: -O2 -ffp-contract=off -fno-fast-math -- the reference's source
semantics, one rounding per operation (SURVEY.md H4's parity target).
-std=c++14 is the level the reference's project builds at (it sets no
LanguageStandard: MSVC's default).  One line of the reference has no defined
meaning at that level: read_ply numbers a leaf with
`leafs[i].tri_list_index = offset + i++` (TD/read_ply.cpp:90,112,136), an
unsequenced read and write of i (C++17 defines it: right operand first, the
store goes to leaf i + 1, which is also what clang does at every level).
Nothing here relies on it: the tests take leaf numbers from the oracle's
reader and compare read_ply's points and boxes only.
-fms-extensions / -fms-compatibility accept the MSVC dialect (members of a
dependent base named without this->); -Wno-error=address-of-temporary: the
address of a temporary, which MSVC allows.
-ftrivial-auto-var-init=zero applies to every translation unit of the
reference, not to one variable: any automatic variable read before it is
written reads as zero.  The one such read known from the source is the upper
half of vector_norm's {float; s64} union (TD/vector.cpp:16-19, H6), whose
lowest bit is shifted into the seed; the flag makes the build say "zero" there
as the oracle does.  AddressSanitizer does not see uninitialised reads, so the
flag could hide another one.  Checked when this recipe was written: with
=pattern and with no such flag at all, tests/test_ref_cpu.py passes unchanged
(rabbit fixture render left out), so no compared result depends on the flag.

A second build of the same sources with -fsanitize=address and
oracle/ref_asan_main.cpp is the stand-alone program oracle/_ref/ref_asan.

Where the reference tree is absent (a GPU host, which receives oracle/_ref/
as built) build() is a no-op.
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
SRC = os.path.join(OUT, "src")
SHIM = os.path.join(HERE, "ref_shim")
LIB_PATH = os.path.join(OUT, "libref.so")
ASAN_PATH = os.path.join(OUT, "ref_asan")
STAMP = os.path.join(OUT, "inputs.sha256")

REF_SUBDIR = "TEST_Dungeonrun"
UNITS = ["Trixel.cu", "Camera.cu", "Quaternion.cu", "Camera.cpp", "Quaternion.cpp", "vector.cpp", "Object.cpp",
         "Color.cpp", "Input.cpp", "read_ply.cpp"]       # not WinMain.cpp, not window_functions.cpp
SOURCE_EXT = (".h", ".cuh", ".cu", ".cpp")
HARNESS = os.path.join(HERE, "ref_harness.cpp")
ASAN_MAIN = os.path.join(HERE, "ref_asan_main.cpp")

# (-fms-compatibility-version: char16_t and friends are keywords; -fgnuc-version and
#  __STDC__: what glibc's and libstdc++'s headers ask of a compiler, which MS mode drops)
COMMON = ["-std=c++14", "-ffp-contract=off", "-fno-fast-math", "-fms-extensions", "-fms-compatibility",
          "-fms-compatibility-version=19.33", "-fgnuc-version=4.2.1", "-D__STDC__=1",
          "-ftrivial-auto-var-init=zero", "-Wno-error=address-of-temporary", "-pthread", "-w", "-I", SHIM, "-I", SRC]
LIB_FLAGS = ["-O2", "-fPIC"]
ASAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address"]


def reference_dir() -> str:
    return os.path.join(os.environ.get("RT_REFERENCE_DIR", "/root/reference"), REF_SUBDIR)


def have_reference() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), UNITS[0]))


def compiler() -> str:
    """clang++: the dialect flags above are clang's."""
    for c in (os.environ.get("RT_REF_CXX"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++",
              "/opt/rocm/lib/llvm/bin/clang++"):
        if c and (os.path.isfile(c) or shutil.which(c)):
            return c
    raise RuntimeError("oracle/ref_build.py needs clang++ (set RT_REF_CXX)")


_OPEN = re.compile(r"\b([A-Za-z_]\w*)\s*<<\s*<")
_CLOSE = re.compile(r">>\s*>\s*\(")


def _split_top(s: str):
    """Split at the commas outside every bracket."""
    parts, depth, cur = [], 0, []
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    parts.append("".join(cur))
    return [p.strip() for p in parts]


def rewrite_launches(text: str) -> str:
    """`k <<< g, b >>> (` -> `REF_LAUNCH(k, g, b)(` (the chevrons may hold blanks)."""
    out, pos = [], 0
    while True:
        m = _OPEN.search(text, pos)
        if not m:
            break
        c = _CLOSE.search(text, m.end())
        cfg = text[m.end():c.start()] if c else ""
        parts = _split_top(cfg)
        if not c or "\n" in cfg or ";" in cfg or len(parts) != 2:
            raise RuntimeError(f"unrecognised kernel launch near: {text[m.start():m.start() + 80]!r}")
        out.append(text[pos:m.start()])
        out.append(f"REF_LAUNCH({m.group(1)}, {parts[0]}, {parts[1]})(")
        pos = c.end()
    out.append(text[pos:])
    return "".join(out)


_SPEC = re.compile(r"^(?=[A-Za-z_])(?!template\b)([\w:]+[\s*&]+)([A-Za-z_]\w*<[^<>;(){}]*>::~?[A-Za-z_]\w*\s*\()", re.M)


def rewrite_specializations(text: str) -> str:
    """`R C<A>::f(` at the start of a line -> `template<> R C<A>::f(`, unless the
    line before it is a template header.  Blanks in the pattern include line
    breaks, so a definition split after its return type or inside its
    brackets is found too; one that the pattern misses does not pass
    silently: clang refuses it and build() raises with its message."""
    def sub(m):
        before = text[:m.start()].rstrip().rsplit("\n", 1)[-1].strip()
        return m.group(0) if before.startswith("template") else "template<> " + m.group(0)
    return _SPEC.sub(sub, text)


def _inputs_digest(ref: str, cxx: str) -> str:
    h = hashlib.sha256()
    files = [os.path.join(ref, f) for f in sorted(os.listdir(ref)) if f.endswith(SOURCE_EXT)]
    files += [os.path.join(SHIM, f) for f in sorted(os.listdir(SHIM))] + [HARNESS, ASAN_MAIN, os.path.abspath(__file__)]
    for p in files:
        with open(p, "rb") as fp:
            h.update(os.path.basename(p).encode() + b"\0" + fp.read() + b"\0")
    h.update(cxx.encode())
    return h.hexdigest()


def _run(cmd, verbose):
    if verbose:
        print("+", " ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout}")


def build(verbose: bool = False, force: bool = False):
    """-> the path of libref.so, or None where neither it nor the reference tree exists."""
    if not have_reference():
        return LIB_PATH if os.path.exists(LIB_PATH) else None
    ref, cxx = reference_dir(), compiler()
    digest = _inputs_digest(ref, cxx)
    if not force and os.path.exists(LIB_PATH) and os.path.exists(ASAN_PATH) and os.path.exists(STAMP):
        with open(STAMP) as fp:
            if fp.read().strip() == digest:
                return LIB_PATH
    for d in (SRC, os.path.join(OUT, "obj"), os.path.join(OUT, "obj_asan")):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    for f in sorted(os.listdir(ref)):
        if f.endswith(SOURCE_EXT):
            with open(os.path.join(ref, f), encoding="utf-8", errors="surrogateescape") as fp:
                text = fp.read()
            with open(os.path.join(SRC, f), "w", encoding="utf-8", errors="surrogateescape") as fp:
                fp.write(rewrite_specializations(rewrite_launches(text)))
    units = [os.path.join(SRC, u) for u in UNITS] + [HARNESS]
    jobs = []
    for sub, flags, extra in (("obj", LIB_FLAGS, []), ("obj_asan", ASAN_FLAGS, [ASAN_MAIN])):
        for u in units + extra:
            o = os.path.join(OUT, sub, os.path.basename(u) + ".o")
            jobs.append(([cxx, *COMMON, *flags, "-x", "c++", "-c", u, "-o", o], o, sub))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda j: _run(j[0], verbose), jobs))
    objs = lambda sub: [o for _, o, s in jobs if s == sub]  # noqa: E731
    _run([cxx, "-shared", "-pthread", "-o", LIB_PATH + ".tmp", *objs("obj")], verbose)
    _run([cxx, "-fsanitize=address", "-pthread", "-o", ASAN_PATH + ".tmp", *objs("obj_asan")], verbose)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    os.replace(ASAN_PATH + ".tmp", ASAN_PATH)
    with open(STAMP, "w") as fp:
        fp.write(digest + "\n")
    return LIB_PATH


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv))
