"""tools/isa_vmcnt_audit.py on a short hand-written listing: the tick loop is found inside the item loop, every vmcnt wait of it is
listed with the loads / stores issued since the previous one (the loop walked as a ring), its barrier count, its block and whether
it lies in the window between the loop's first output store and the first load behind the loop's top."""
import importlib.util
import os

import pytest

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "isa_vmcnt_audit.py")
_spec = importlib.util.spec_from_file_location("isa_vmcnt_audit", _PATH)
audit_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(audit_mod)

LISTING = """\
	.text
_Z5otherv:                              ; @_Z5otherv
	global_store_dword v0, v1, s[0:1]
	s_waitcnt vmcnt(0)
	s_endpgm
.Lfunc_end0:
_Z4tickILi128EEvv:                      ; @_Z4tickILi128EEvv
; %bb.0:
	global_load_dword v9, v0, s[0:1]
	s_waitcnt vmcnt(0) lgkmcnt(0)
.LBB1_1:                                ; item loop
	s_barrier
	global_load_dwordx2 v[2:3], v0, s[2:3] sc1
.LBB1_2:                                ; tick loop
	s_waitcnt lgkmcnt(0)
	s_barrier
	v_add_f64 v[4:5], v[2:3], v[2:3]
	s_waitcnt vmcnt(0)                      ; early: a reused load register
	ds_read_b64 v[6:7], v1
	s_barrier
	global_load_dwordx2 v[10:11], v0, s[4:5]
	s_cbranch_execz .LBB1_4
; %bb.3:
	global_load_dwordx2 v[12:13], v0, s[6:7]
.LBB1_4:
	s_barrier
	s_waitcnt vmcnt(1)
	v_mov_b32_e32 v20, v10
	global_store_dword v0, v20, s[8:9]
	global_store_dwordx4 v0, v[4:7], s[8:9] offset:16
	s_waitcnt vmcnt(0) lgkmcnt(0)
	ds_write_b64 v1, v[12:13]
	s_barrier
	s_cbranch_scc1 .LBB1_2
; %bb.5:
	global_store_dword v0, v1, s[10:11]
	s_waitcnt vmcnt(0)
	s_barrier
	s_cbranch_scc0 .LBB1_1
; %bb.6:
	s_endpgm
.Lfunc_end1:
	.size	_Z4tickILi128EEvv, .Lfunc_end1-_Z4tickILi128EEvv
"""


def test_audit_finds_the_tick_loop_and_its_waits():
    res = audit_mod.audit(LISTING.split("\n"), "_Z4tickILi128E")
    assert res["kernel"] == "_Z4tickILi128EEvv"
    assert res["loop_block"] == ".LBB1_2"                 # 4 of the kernel's 6 barriers; the item loop holds all of them but is larger
    waits = res["waits"]
    assert [w["vmcnt"] for w in waits] == [0, 1, 0]       # (the lgkmcnt-only wait is no vmcnt wait)
    assert [w["block"] for w in waits] == [".LBB1_2", ".LBB1_4", ".LBB1_4"]
    assert [w["barrier"] for w in waits] == [1, 3, 3]
    # the ring: the first wait sees nothing since the loop's last wait; text order counts the skipped block's load
    assert [(w["loads"], w["stores"]) for w in waits] == [(0, 0), (2, 0), (0, 2)]
    # first load behind the top at pos 6, first store at pos 12: the early wait and the one behind the stores drain stores
    assert (res["first_load"], res["first_store"]) == (6, 12)
    assert [w["window"] for w in waits] == [True, False, True]
    assert [w["pos"] for w in waits] == [3, 10, 14]
    text = audit_mod.report(res)
    assert "vmcnt waits in the loop: 3, of them inside the store window: 2" in text
    assert len(text.split("\n")) == 3 + 3 + 1


def test_audit_named_loop_and_errors():
    res = audit_mod.audit(LISTING.split("\n"), "_Z4tick", header=".LBB1_1")
    assert res["loop_block"] == ".LBB1_1" and len(res["waits"]) == 4     # + the item's drain in front of its publish
    assert res["waits"][-1]["stores"] == 1 and res["waits"][-1]["window"]
    with pytest.raises(SystemExit):
        audit_mod.audit(LISTING.split("\n"), "_Z")                      # two kernels
    with pytest.raises(SystemExit):
        audit_mod.audit(LISTING.split("\n"), "_Z5other")                # no loop
    with pytest.raises(SystemExit):
        audit_mod.audit(LISTING.split("\n"), "_Z4tick", header=".LBB1_4")
