"""tools/asm_diff.py compares WHOLE kernels: a kernel with an early exit holds more than one s_endpgm, and its body ends at .Lfunc_end<N>, not at the first of them.
Synthetic listings in the shape `hipcc -S --cuda-device-only` emits (kernel descriptor and padding between the last instruction and the end label); no GPU, no hipcc."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_diff  # noqa: E402

K1, K2 = "_Z8k_one_kernelILi0EEvPf", "_Z8k_two_kernelILi0EEvPf"


def kernel(name, n, tail, pad=()):
    """Two program ends: an early exit after 3 instructions, then `tail` and the last s_endpgm (5 + len(tail) instructions in all)."""
    head = [f"{name}:                ; @{name}", "; %bb.0:", "\ts_load_dword s3, s[0:1], 0x24", "\ts_cmp_lt_i32 s3, 1", f"\ts_cbranch_scc0 .LBB{n}_2", "; %bb.1:",
            "\ts_endpgm", f".LBB{n}_2:"]
    end = ["\ts_endpgm", *(f"\t{p}" for p in pad), "\t.section\t.rodata,\"a\",@progbits", f"\t.amdhsa_kernel {name}", "\t\t.amdhsa_next_free_vgpr 10", "\t.end_amdhsa_kernel",
           "\t.text", f".Lfunc_end{n}:", f"\t.size\t{name}, .Lfunc_end{n}-{name}"]
    return head + [f"\t{t}" for t in tail] + end


def listing(tmp_path, fname, *ks):
    p = tmp_path / fname
    p.write_text("\t.text\n" + "\n".join(line for k in ks for line in k) + "\n")
    return str(p)


TAIL = ["v_mov_b32_e32 v1, 0", "global_store_dword v1, v0, s[4:5]"]


def test_a_difference_after_the_first_program_end_is_reported(tmp_path, capsys):
    old = listing(tmp_path, "old.s", kernel(K1, 0, TAIL), kernel(K2, 1, TAIL))
    new = listing(tmp_path, "new.s", kernel(K1, 0, TAIL), kernel(K2, 1, ["v_mov_b32_e32 v1, 1", TAIL[1]]))
    assert asm_diff.main(old, new, "_kernel") == 1
    out = capsys.readouterr().out.splitlines()
    assert out[0] == f"{K1}: 7 -> 7 instructions, IDENTICAL"
    assert out[1].startswith(f"{K2}: 7 -> 7 instructions, 1 differing lines, first: [('v_mov_b32_e32 v1, 0', 'v_mov_b32_e32 v1, 1')]")
    # a tail of another length alone is a difference too
    new = listing(tmp_path, "new2.s", kernel(K1, 0, TAIL), kernel(K2, 1, TAIL + ["s_nop 0", "v_mov_b32_e32 v2, 0"]))
    assert asm_diff.main(old, new, "_kernel") == 1
    assert f"{K2}: 7 -> 9 instructions, 1 differing lines, first: [('s_endpgm', 's_nop 0')]" in capsys.readouterr().out


def test_identical_listings_report_the_full_instruction_count(tmp_path, capsys):
    """Block numbering (the kernel's position in its file) and the padding before the end label do not count."""
    old = listing(tmp_path, "old.s", kernel(K1, 0, TAIL), kernel(K2, 1, TAIL))
    new = listing(tmp_path, "new.s", kernel(K2, 0, TAIL, pad=["s_nop 0", "s_nop 0"]), kernel(K1, 1, TAIL, pad=["s_code_end"]))
    assert asm_diff.main(old, new, "_kernel") == 0
    assert capsys.readouterr().out.splitlines() == [f"{K1}: 7 -> 7 instructions, IDENTICAL", f"{K2}: 7 -> 7 instructions, IDENTICAL"]
    assert [len(v) for v in asm_diff.kernels(old, "k_one").values()] == [7]


def test_a_kernel_missing_on_one_side_fails(tmp_path, capsys):
    old = listing(tmp_path, "old.s", kernel(K1, 0, TAIL), kernel(K2, 1, TAIL))
    new = listing(tmp_path, "new.s", kernel(K1, 0, TAIL))
    assert asm_diff.main(old, new, "_kernel") == 1
    assert f"{K2}: not in {new}" in capsys.readouterr().out
    assert asm_diff.main(new, old, "_kernel") == 0          # a kernel that is only new is listed, as before
    assert f"{K2}: new (7 instructions)" in capsys.readouterr().out


def test_a_kernel_without_its_end_label_fails_loudly(tmp_path):
    """A truncated listing must not drop its last kernel or run it into the next one."""
    whole = kernel(K1, 0, TAIL) + kernel(K2, 1, TAIL)
    cut_last = listing(tmp_path, "cut_last.s", [ln for ln in whole if ".Lfunc_end1" not in ln])
    cut_first = listing(tmp_path, "cut_first.s", [ln for ln in whole if ".Lfunc_end0" not in ln])
    ok = listing(tmp_path, "ok.s", whole)
    for bad, name in ((cut_last, K2), (cut_first, K1)):
        with pytest.raises(SystemExit, match=name):
            asm_diff.main(ok, bad, "_kernel")
