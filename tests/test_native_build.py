"""The prerequisite lists of the tests' native helpers (tests/native.mk, the Makefile of each directory) against the compiler's
own view: a library must be out of date, by `make`'s judgement, as soon as ANY file its translation unit reads is newer --
every header `g++ -MM` reports inside the repository, the source itself and tests/native.mk.  Nothing is touched: `make -q -W
<file>` answers "would you rebuild if <file> had just changed".  A library that is not rebuilt after an edit of a header runs
the CPU tests, and travels to the GPU, with code that is no longer in the tree."""
import os
import shlex
import subprocess

import pytest

from tests import native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# (directory, library, the library whose compile line says what the translation unit is)
HOST = [(d, lib, lib) for d, lib in (
    ("emu", "libpveenv_emu.so"), ("emu_wide", "libpveenv_emu_wide.so"), ("emu_diag", "libpveenv_emu_diag.so"),
    ("noise_host", "libnoise_host.so"), ("critic_host", "libcritic_host.so"), ("nstep_host", "libnstep_host.so"),
    ("replay_host", "libreplay_host.so"), ("learner_host", "liblearner_host.so"), ("learner_host", "liblearner_host_sub.so"),
    ("learner_wide_host", "liblearner_wide_host.so"), ("prio_host", "libprio_host.so"), ("arrivals_host", "libarrivals_host.so"),
    ("stats_host", "libstats_host.so"), ("math_probe", "libpve_math_probe_host.so"))]
# the device flavour of the probe is the same source: its headers are those of the host flavour (-x c++)
CASES = HOST + [("math_probe", "libpve_math_probe_hip.so", "libpve_math_probe_host.so")]


def make(directory, *args):
    return subprocess.run(["make", "-s"] + list(args), cwd=os.path.join(native.TESTS_DIR, directory), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True)


def files_read(directory, library):
    """Every file under the repository that the compiler reads for `library`: its own compile line (make -n -B: the target's
    flags and defines), linking taken out, -MM put in.  Paths relative to the directory, as its Makefile spells them."""
    here = os.path.join(native.TESTS_DIR, directory)
    p = make(directory, "-n", "-B", library)
    assert p.returncode == 0, p.stdout
    compile_lines = [ln for ln in p.stdout.splitlines() if " -shared " in ln and (" -o %s " % library) in ln + " "]
    assert len(compile_lines) == 1, p.stdout
    words = shlex.split(compile_lines[0])
    at = words.index("-o")
    words = [w for w in words[:at] + words[at + 2:] if w not in ("-shared", "-lm")] + ["-MM"]
    out = subprocess.run(words, cwd=here, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    deps = shlex.split(out.replace("\\\n", " ").split(":", 1)[1])
    inside = [os.path.realpath(os.path.join(here, d)) for d in deps]
    inside = sorted({f for f in inside if f.startswith(ROOT + os.sep)})
    assert any(f.endswith("pve_types.h") for f in inside), out              # (the parse found the headers)
    return [os.path.relpath(f, here) for f in inside]


@pytest.mark.parametrize("directory,library,unit", CASES, ids=[c[1] for c in CASES])
def test_library_is_stale_after_any_file_it_reads(directory, library, unit):
    native.build(directory, library)                       # a failure to build is an error
    p = make(directory, "-q", library)
    assert p.returncode == 0, "%s is not up to date right after its build: %s" % (library, p.stdout)
    files = files_read(directory, unit) + ["../native.mk"]
    print("NATIVE_BUILD", library, len(files), "files")
    kept = [f for f in files if make(directory, "-q", "-W", f, library).returncode != 1]
    assert kept == [], "%s is not rebuilt after a change of %s" % (library, kept)
