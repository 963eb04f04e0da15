"""The one loader of the tests' native helpers (the CPU emulators, the g++ builds of single headers, the math probe).  How they
are built is tests/native.mk's business and whether one is stale is `make`'s: this module asks it once per process and
library, which costs nothing when __graft_entry__.build() (or `make -C tests`) has been there.  A failure to build is an error."""
import ctypes as C
import functools
import os
import subprocess

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def build(directory, library):
    """`make` tests/<directory>/<library> -> its path"""
    subprocess.check_call(["make", "-C", os.path.join(TESTS_DIR, directory), "-s", library])
    return os.path.join(TESTS_DIR, directory, library)


@functools.lru_cache(maxsize=None)
def load(directory, library, declare=None):
    """The CDLL of tests/<directory>/<library>, handed through declare(lib) -> lib (the ctypes signatures, which stay next to
    the wrappers that use them) when it is first loaded."""
    lib = C.CDLL(build(directory, library))
    return declare(lib) if declare else lib


def load_emulator(directory, library):
    """An emulator of the product library: the product's own declarations of the C ABI"""
    from pve_mcc_amd import _capi
    return load(directory, library, _capi._declare)
