"""tools/asm_mix.py on a small hand-written listing (CPU only): functions are
found by their .type / label / .size, instructions are classed by mnemonic
prefix, and only innermost backward-branch ranges count as loops."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LISTING = """
\t.text
\t.type\t_Z3fooi,@function
_Z3fooi:                                ; @_Z3fooi
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tv_mov_b32_e32 v0, 0
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
\tv_fma_f64 v[2:3], v[4:5], v[6:7], v[2:3]
\tds_read_b64 v[4:5], v1
\tglobal_load_dwordx2 v[6:7], v8, s[0:1]
\ts_nop 1
\ts_cbranch_scc1 .LBB0_2
; %bb.3:
\tv_add_f64 v[2:3], v[2:3], 1.0
\ts_cbranch_vccnz .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z3fooi, .Lfunc_end0-_Z3fooi
; codeLenInByte = 96
\t.type\t_Z3barv,@function
_Z3barv:
\ts_setpc_b64 s[30:31]
.Lfunc_end1:
\t.size\t_Z3barv, .Lfunc_end1-_Z3barv
"""


def test_functions_classes_and_innermost_loops(tmp_path, capsys):
    import asm_mix
    p = tmp_path / "x.s"
    p.write_text(LISTING)
    fns = asm_mix.functions(str(p))
    assert [f[0] for f in fns] == ["_Z3fooi", "_Z3barv"]
    name, items, nbytes = fns[0]
    assert nbytes == 96
    c = asm_mix.mix(items)
    assert c == {"f64": 2, "valu": 1, "salu": 4, "wait": 1, "nop": 1, "lds": 1, "vmem": 1,
                 "other": 0}
    loops = asm_mix.innermost_loops(items)
    assert len(loops) == 1  # the outer loop contains the inner one
    inner = asm_mix.mix(items[loops[0][0]:loops[0][1] + 1])
    assert inner["f64"] == 1 and inner["lds"] == 1 and inner["vmem"] == 1 and sum(inner.values()) == 5
    assert asm_mix.main([str(p), "--match", "foo"]) == 0
    out = capsys.readouterr().out
    assert "_Z3fooi" in out and "_Z3barv" not in out and "loop @.LBB0_2" in out
    # the enclosing loop: both levels, the outer one around the inner one's instructions
    every = asm_mix.all_loops(items)
    assert len(every) == 2 and [asm_mix.depth(l, every) for l in every] == [0, 1]
    assert sum(asm_mix.mix(items[every[0][0]:every[0][1] + 1]).values()) == 8
    assert asm_mix.main([str(p), "--match", "foo", "--enclosing"]) == 0
    out = capsys.readouterr().out
    assert "loop d0 @.LBB0_1" in out and "loop d1 @.LBB0_2" in out
