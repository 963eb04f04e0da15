# How the tests' native helpers are built; included by the Makefile of every directory under tests/ that builds one
# (paths are relative to such a directory).  tests/Makefile builds them all, tests/native.py loads them.
CXX ?= g++
CSRC = ../../pve-mcc_for_unsignalized_intersection_amd/csrc
WARN = -Wall -Wno-unused-function -Wno-unknown-pragmas
# the CPU emulators (tests/emu hands this set to tests/math_probe's host flavour)
EMU_CXXFLAGS = -O2 -g -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -fno-strict-aliasing $(WARN)
# the g++ builds of single host+device headers
SHIM_CXXFLAGS = -O2 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math $(WARN)
# Every target depends on every header of the product, whichever it includes today: a rebuild too many costs seconds, a
# library older than a header it includes runs the tests on code that is no longer there (tests/test_native_build.py
# holds this list to the compiler's -MM).
PREREQS = $(wildcard $(CSRC)/*.h $(CSRC)/*.inc) $(wildcard ../../include/*.h) ../native.mk Makefile
