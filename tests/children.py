"""Everything in the tests that starts a process: traced model runs (rocprofv3 --kernel-trace), the plain-C examples, the children that
import torch before the library (graph capture), and the host-only builds (syntax checks, the sanitized host-check programs).

One rule for every child that may touch the GPU: after one of them ended at its time limit or on a signal, no further one is started
in this session -- traced(), run_example() and python_child() fail with "not started: ...".  A child that merely exits 1 (a failed
assertion) leaves the rule alone.  Host-only builds are not subject to it."""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import kernel_inventory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "optimized-number-theoretic-transform-implementations_amd", "csrc")

_UNCLEAN = []  # what did not end cleanly: at most one entry, nothing is started after it


def _reset():
    """for the latch's own test only"""
    del _UNCLEAN[:]


def _run(what, cmd, seconds=None):
    """the one place a GPU child is started; trips the latch on a time limit, an abort, a segmentation fault or any signal"""
    if _UNCLEAN:
        pytest.fail("not started: %s did not end cleanly" % _UNCLEAN[0])
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    except subprocess.TimeoutExpired as e:
        _UNCLEAN.append(what)
        pytest.fail("%s ran into its limit of %d s:\n%s\n%s" % (what, seconds, _tail(e.stdout), _tail(e.stderr)))
    if r.returncode in (124, 137, 134, 139) or r.returncode < 0:
        _UNCLEAN.append(what)
    return r


def _tail(text, n=4000):
    if isinstance(text, bytes):
        text = text.decode(errors="replace")
    return (text or "")[-n:]


def rocprofv3():
    exe = "/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else shutil.which("rocprofv3")
    if not exe:
        pytest.fail("rocprofv3 is not on this machine: the launch proofs need its kernel trace")
    return exe


def trace_names(directory, log=""):
    """the normalised kernel names of the *kernel_trace.csv files under a directory, one entry per dispatch, in order"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "the kernel trace wrote no CSV:\n" + log[-2000:]
    names = []
    for f in files:
        with open(f, newline="") as fh:
            names += [row["Kernel_Name"] for row in csv.DictReader(fh)]
    mangled = sorted({n for n in names if n.startswith("_Z")})
    dem = dict(zip(mangled, kernel_inventory.demangle(mangled)))
    return [kernel_inventory.normalise(dem.get(n, n)) for n in names]


def traced(script, args, seconds):
    """run `python3 SCRIPT ARGS` in a fresh child process under a kernel trace: the normalised kernel names it launched, one entry
    per dispatch"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(seconds), rocprofv3(), "--kernel-trace", "--output-format", "csv", "-d", d, "--",
               sys.executable, script] + list(args)
        r = _run("the traced run of %s %s" % (os.path.basename(script), " ".join(args)), cmd)
        assert r.returncode == 0, "traced run failed (exit %d):\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
        return trace_names(d, r.stderr)


STRICT = ("-Wall", "-Wextra", "-Werror")


def gcc(*args):
    """the C compiler as every test calls it: optimised gnu11 against the public header"""
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-I" + INCLUDE] + [str(a) for a in args])


def build_example(lib, name, *extra):
    """examples/NAME.c against the public header and the library (extra: further compiler arguments) -> build/NAME"""
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.dirname(lib.LIB_PATH)
    gcc(os.path.join(ROOT, "examples", name + ".c"), "-L" + libdir, "-lntt_mi355x", "-Wl,-rpath," + libdir, *extra, "-o", exe)
    return exe


def run_example(lib, name, seconds=120, extra=()):
    """build and run a plain-C example under its time limit: its stdout"""
    exe = build_example(lib, name, *extra)
    r = _run("the example " + name, ["timeout", "-k", "10", str(seconds), exe])
    assert r.returncode == 0, "%s failed (exit %d):\n%s\n%s" % (name, r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    return r.stdout


def python_child(code, seconds=300, marker="graph ok"):
    """run a script in a fresh interpreter (a child of its own, so that it can import torch before the library), the repository and
    tests/ on its path; it has to exit 0 and print the marker"""
    pre = "import sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (ROOT, os.path.join(ROOT, "tests"))
    r = _run("a python child", [sys.executable, "-c", pre + code], seconds)
    assert r.returncode == 0 and marker in r.stdout, "child failed (exit %d):\n%s\n%s" % (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def syntax_check(src):
    """compile a source text against the public header alone, as C (gnu11) and as C++17, warnings as errors"""
    for comp, std, lang in (("gcc", "-std=gnu11", "c"), ("g++", "-std=c++17", "c++")):
        subprocess.run([comp, std, "-Wall", "-Wextra", "-Werror", "-Wno-address", "-fsyntax-only", "-I" + INCLUDE, "-x", lang, "-"],
                       input=src, text=True, check=True)


# host code only, every sanitizer flag bound to the host side: nothing is built for the GPU
HOST_SANITIZE = ("-O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined "
                 "-Xarch_host -fno-sanitize-recover=all")


def build_host_check(name, flags=HOST_SANITIZE):
    """tests/NAME.cpp, a stand-alone host program over the csrc headers -> build/NAME"""
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only"] + flags.split() + ["-I" + CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe
