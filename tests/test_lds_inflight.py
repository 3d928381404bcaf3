"""benchmarks/lds_inflight.py: the lgkmcnt walk over a hand-written
fragment.  DS and scalar-memory instructions increment the counter, a wait
that names lgkmcnt clamps it, everything else is ignored."""

import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location(
    "lds_inflight", os.path.join(REPO, "benchmarks", "lds_inflight.py"))
lds_inflight = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lds_inflight)

ASM = """
	.text
	.globl	_Z3fooPj
_Z3fooPj:                               ; @_Z3fooPj
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0      ; 1 outstanding
	v_perm_b32 v1, v0, v2, s6
	ds_read_b32 v3, v1                      ; 2
	ds_read_b32 v4, v1 offset:128           ; 3
	s_waitcnt vmcnt(0)                      ; not an lgkm wait
	ds_read_b32 v5, v1 offset:256           ; 4: the peak
	s_waitcnt lgkmcnt(2)                    ; reached with 4 -> 2
.LBB0_1:
	v_xor_b32_e32 v3, v3, v4
	ds_write_b32 v1, v3                     ; 3
	s_waitcnt vmcnt(0) lgkmcnt(0)           ; reached with 3 -> 0
	s_waitcnt lgkmcnt(0)                    ; reached with 0
	s_endpgm
.Lfunc_end0:
	.size	_Z3fooPj, .Lfunc_end0-_Z3fooPj
_Z3barv:
	ds_read_b32 v0, v1
	s_waitcnt lgkmcnt(0)
	s_endpgm
.Lfunc_end1:
"""


def test_walk_counts():
    (name, r), = lds_inflight.analyse(ASM, "foo")
    assert name == "_Z3fooPj"
    assert r["ds_read_b32"] == 3
    assert r["waits"] == 3
    assert r["peak"] == 4
    assert r["mean"] == (4 + 3 + 0) / 3
    # buckets 0, 1-2, 3-4, 5-8, ...
    assert r["hist"][:3] == [1, 0, 2] and sum(r["hist"]) == 3


def test_pattern_selects_kernels():
    both = lds_inflight.analyse(ASM, ".")
    assert [n for n, _ in both] == ["_Z3fooPj", "_Z3barv"]
    assert both[1][1]["ds_read_b32"] == 1 and both[1][1]["peak"] == 1
    assert lds_inflight.analyse(ASM, "nothing") == []


def test_cli(tmp_path, capsys):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    assert lds_inflight.main([str(p), "bar"]) == 0
    out = capsys.readouterr().out
    assert "_Z3barv" in out and "foo" not in out
    assert "ds_read_b32 1  waits 1" in out
    assert lds_inflight.main([str(p), "nothing"]) == 1
