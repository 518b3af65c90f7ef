"""CPU checks of the two hand-placed GEMM loops (no GPU): the committed .inc files are what the generators produce, and the built code objects keep the contract the
inline-asm statements rely on -- gemm_a4_kernel's accumulators live in a[0:255] ACROSS statements the compiler knows nothing about, so a compiler-inserted
v_accvgpr_write (an AGPR spill) anywhere in that kernel, or any scratch use, would silently corrupt a tile (cdna_hip_programming.md 5.7 item 4)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_budget  # noqa: E402

SO = os.path.join(ROOT, "grounded-video-llm_amd", "libgvl.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.parametrize("gen", ["gen_gemm4_loop.py", "gen_gemm4p.py"])
def test_generated_loops_are_up_to_date(gen):
    env = {k: v for k, v in os.environ.items() if not k.startswith("GVL_A4P_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen), "--check"], env=env)
    assert r.returncode == 0, f"grounded-video-llm_amd/csrc/*.inc is stale: run python tools/{gen}"


@pytest.fixture(scope="module")
def disasm():
    if not (os.path.exists(SO) and os.path.exists(OBJDUMP)):
        pytest.skip("libgvl.so not built / no llvm-objdump")
    out = {}
    import tempfile
    for elf in isa_budget.code_objects(SO):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf); f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", txt, re.S | re.M):
            if "gemm_a4" in m.group(1):
                out[m.group(1)] = m.group(2)
    assert out, "no 4-wave GEMM kernel found in libgvl.so"
    return out


def test_four_wave_kernels_keep_the_accumulator_file_to_the_asm(disasm):
    ks = isa_budget.kernels(SO)
    seen = {"a4": 0, "a4p": 0}
    for name, body in disasm.items():
        if name.endswith(".kd"):
            continue
        r = ks[name]
        assert r[".vgpr_spill_count"] == 0 and r[".private_segment_fixed_size"] == 0, (name, r)
        assert r[".agpr_count"] == 256, (name, r)
        reads, writes = body.count("v_accvgpr_read_b32"), body.count("v_accvgpr_write")
        assert writes == 0, f"{name}: {writes} compiler-inserted v_accvgpr_write"
        mfma = body.count("v_mfma_f32_32x32x16_bf16")
        if "gemm_a4p" in name:
            seen["a4p"] += 1
            # first-tile statement + pipelined statement: a drain of 256 each; the epilogues with NARROW statements (N = 1408's half column tile: 128 x 64 per wave)
            # carry two more drains of 128 and bodies of 32 MFMAs
            narrow = "Li184E" in name
            assert reads == (768 if narrow else 512), f"{name}: {reads} v_accvgpr_read"
            assert mfma % (32 if narrow else 64) == 0 and mfma >= 2 * 4 * 64, (name, mfma)
        else:
            seen["a4"] += 1
            assert reads == 256, f"{name}: {reads} v_accvgpr_read (one epilogue of 256 expected)"
            assert mfma == 4 * 64, (name, mfma)                                                         # FIRST, STEADY, PENULT, LAST bodies
    assert seen["a4"] >= 13 and seen["a4p"] >= 8, seen


# ---- operand contract of the inline-asm statements ---------------------------------------------------------------------------------------------------------------
# Every statement of the two generated streams is parsed instruction by instruction and held against the constraint lists its wrapper (gvl_gemm4.hip /
# gvl_gemm4p.hip) hands the compiler:
#   * every VGPR / SGPR / AGPR (and vcc, scc) an instruction WRITES is declared as an output, an in/out operand or a clobber -- a register the compiler takes for an
#     input-only operand may be reused by it after the statement, so a silent write is a wrong tile waiting for a compiler bump;
#   * every register READ before its first write in the statement is an input, an in/out operand or a documented cross-statement resident: the AGPR accumulators
#     (a[0:255] live across the statements by design, see the module docstring) and m0 (saved on entry, restored on exit: checked).
# Control flow: the text is walked in program order (the k loop and the forward skip over the steady body only repeat / leave out writes of registers the FIRST body
# has already written); the one real fork -- the narrow / wide halves of the statements that hold both codes -- is walked as two paths.
# Which operand an instruction writes comes from a table of the mnemonics that occur; a mnemonic missing from it FAILS the audit.
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")
# mnemonic -> (number of leading destination operands, the destination is also read, implicit reads, implicit writes)
_VALU = ("v_cvt_pk_bf16_f32 v_lshlrev_b32 v_lshrrev_b32 v_and_b32 v_xor_b32 v_mul_f32 v_add_u32 v_add_f32 v_add_f32_dpp v_lshl_add_u32 v_lshl_or_b32 v_pk_add_f32 "
         "v_pk_mul_f32 v_pk_fma_f32 v_mov_b32 v_rcp_f32 v_exp_f32 v_min_u32 v_max_u32 v_bfe_u32 v_mbcnt_lo_u32_b32 v_mbcnt_hi_u32_b32 v_accvgpr_read_b32 "
         "v_readfirstlane_b32 v_cndmask_b32 v_mfma_f32_32x32x16_bf16 ds_read_b128 ds_read_b32 s_mov_b32 s_mul_i32").split()
MNEMONICS = {m: (1, False, (), ()) for m in _VALU}
MNEMONICS.update({
    "v_dot2c_f32_bf16": (1, True, (), ()),                                   # d += a.lo b.lo + a.hi b.hi
    "v_cmp_eq_u32": (1, False, (), ()),                                      # the destination is spelled out (vcc)
    "s_add_u32": (1, False, (), ("scc",)), "s_sub_u32": (1, False, (), ("scc",)), "s_xor_b32": (1, False, (), ("scc",)),
    "s_cmp_eq_u32": (0, False, (), ("scc",)), "s_cmp_lg_u32": (0, False, (), ("scc",)),
    "s_cbranch_scc1": (0, False, ("scc",), ()), "s_branch": (0, False, (), ()),
    "s_waitcnt": (0, False, (), ()), "s_nop": (0, False, (), ()), "s_barrier": (0, False, (), ()),
    "buffer_store_dwordx4": (0, False, (), ()), "buffer_store_dword": (0, False, (), ()), "ds_write_b64": (0, False, (), ()), "ds_write_b32": (0, False, (), ()),
    # loads: a register destination unless the `lds` modifier sends the data to LDS at m0 (then every operand is a source)
    "buffer_load_dwordx4": (1, False, (), ()), "buffer_load_dword": (1, False, (), ()),
})
_STATEMENT = re.compile(r"^GVL_A4P?_(TILE_ASM_V\d+|DMA_TILE_ASM|TILE0_E\d+|TILE_E\d+|FLUSH_E\d+)$")


def _macros(text):
    """#define NAME[(params)] body, continuation lines joined -> {NAME: (is_function_like, body)}"""
    text = text.replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(\([^)]*\))?[ \t]*(.*)$", text, re.M):
        out[m.group(1)] = (m.group(2) is not None, m.group(3))
    return out


def _regs(tok):
    """one operand token -> set of registers: ('v', 12), ('s', 40), ('a', 3), ('vcc', 0), ('scc', 0), ('m0', 0), ('op', N) for a %N operand; literals -> empty"""
    tok = tok.strip()
    m = re.fullmatch(r"([vsa])\[(\d+):(\d+)\]", tok)
    if m:
        return {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.fullmatch(r"([vsa])(\d+)", tok)
    if m:
        return {(m.group(1), int(m.group(2)))}
    if tok in ("vcc", "scc", "m0"):
        return {(tok, 0)}
    m = re.fullmatch(r"%(\d+)", tok)
    if m:
        return {("op", int(m.group(1)))}
    if re.fullmatch(r"-?(0x[0-9a-fA-F]+|\d+(\.\d+)?)", tok):
        return set()
    raise AssertionError(f"operand not understood: {tok!r}")


def _split_top(s, sep):
    """split at `sep` outside string literals and brackets"""
    out, depth, cur, q = [], 0, "", False
    for ch in s:
        if ch == '"':
            q = not q
        if not q:
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == sep and depth == 0:
                out.append(cur)
                cur = ""
                continue
        cur += ch
    return out + [cur]


def _instruction(line):
    """-> (mnemonic, writes, reads) of one asm line; None for labels / directives"""
    line = line.strip()
    if not line or line.endswith(":") or line.startswith("."):
        return None
    mn, _, rest = line.partition(" ")
    assert mn in MNEMONICS, f"mnemonic {mn!r} is not in the destination-operand table (tests/test_gemm4_loop_gen.py: MNEMONICS): add it, with the operand it writes"
    ndst, dst_read, imp_r, imp_w = MNEMONICS[mn]
    ops, mods = [], []
    for piece in _split_top(rest, ","):
        words = piece.split()
        if words:
            ops.append(words[0])
            mods += words[1:]
    if mn.startswith("s_cbranch") or mn == "s_branch" or mn in ("s_waitcnt", "s_nop", "s_barrier"):
        ops = []
    if mn.startswith("buffer_load") and "lds" in mods:
        ndst, imp_r, imp_w = 0, ("m0",), ()
    writes, reads = set(), set()
    for k, o in enumerate(ops):
        r = _regs(o)
        if k < ndst:
            writes |= r
            if dst_read:
                reads |= r
        else:
            reads |= r
    reads |= {(x, 0) for x in imp_r}
    writes |= {(x, 0) for x in imp_w}
    return mn, writes, reads


def _paths(lines):
    """program-order walks of a statement: one, or two for the statements that hold a narrow and a wide code behind one branch"""
    wide = [i for i, l in enumerate(lines) if l.startswith(".Lgvl_a4p_wide_")]
    if not wide:
        return [lines]
    w = wide[0]
    br = max(i for i in range(w) if lines[i].startswith("s_branch .Lgvl_a4p_end_"))
    head = next(i for i, l in enumerate(lines) if l.startswith("s_cbranch_scc1 .Lgvl_a4p_wide_"))
    return [lines[:br], lines[:head + 1] + lines[w:]]


def _audit_statement(name, lines, outs, inouts, ins, clobbers):
    """-> list of findings (strings) of one statement against its declared operands"""
    found = []
    resident = {("a", i) for i in range(256)} | {("m0", 0)}
    may_write = outs | inouts | clobbers
    may_read_first = ins | inouts | resident
    for path in _paths(lines):
        written, bad_w, bad_r, m0_saved_in = set(), {}, {}, None
        for ln in path:
            ins_ = _instruction(ln)
            if ins_ is None:
                continue
            mn, w, r = ins_
            for reg in sorted(r - written - may_read_first):
                bad_r.setdefault(reg, ln)
            if mn == "s_mov_b32" and ("m0", 0) in r and ("m0", 0) not in written and m0_saved_in is None:
                m0_saved_in = next(iter(w))
            for reg in sorted(w - may_write):
                if reg == ("m0", 0):
                    continue                                                 # judged as a whole below: saved first, restored last
                bad_w.setdefault(reg, ln)
            written |= w
        if ("m0", 0) in written:
            last = [l for l in path if _instruction(l)][-1]
            ok = m0_saved_in is not None and last == f"s_mov_b32 m0, {m0_saved_in[0]}{m0_saved_in[1]}" and \
                sum(1 for l in path if (_instruction(l) or (0, set(), 0))[1] == {m0_saved_in}) == 1
            if not ok:
                found.append(f"{name}: writes m0 without the save-first / restore-last pair")
        for kind, bad in (("writes", bad_w), ("reads before any write", bad_r)):
            if bad:
                regs = sorted(bad)
                spans = ", ".join(f"{k}{i}" for k, i in regs[:6]) + (f" ... {regs[-1][0]}{regs[-1][1]} ({len(regs)} registers)" if len(regs) > 6 else "")
                msg = f"{name}: {kind} {spans}, declared neither as " + ("output, in/out nor clobber" if kind == "writes" else "input nor in/out") + f"; first: `{bad[regs[0]]}`"
                if msg not in found:
                    found.append(msg)
    return found


def _constraints(section, kind, first_index):
    """one colon-separated section of an asm statement -> (outs, inouts, ins) register sets; generic "v" / "s" operands become ('op', index)"""
    outs, inouts, ins = set(), set(), set()
    k = first_index
    for item in _split_top(section, ","):
        m = re.match(r'\s*"([=+]?)&?(\{[^}]*\}|[a-zA-Z])"\s*\(', item)
        if not m:
            assert not item.strip(), f"constraint not understood: {item!r}"
            continue
        regs = _regs(m.group(2)[1:-1]) if m.group(2).startswith("{") else {("op", k)}
        if kind == "in":
            assert m.group(1) == "", item
            ins |= regs
        elif m.group(1) == "+":
            inouts |= regs
        else:
            assert m.group(1) == "=", item
            outs |= regs
        k += 1
    return outs, inouts, ins, k


def audit_asm_contract(csrc=CSRC, wrappers=(("gvl_gemm4.hip", ("gvl_gemm4_loop.inc",)), ("gvl_gemm4p.hip", ("gvl_gemm4p_loop.inc", "gvl_gemm4p_operands.inc")))):
    """-> (findings, names of the statements audited)"""
    findings, seen = [], []
    for hip, incs in wrappers:
        hip_txt = open(os.path.join(csrc, hip)).read().replace("\\\n", " ")
        mac, inc = {}, incs[0]
        for f in incs:
            if os.path.exists(os.path.join(csrc, f)):
                mac.update(_macros(open(os.path.join(csrc, f)).read()))
        mac.update(_macros(hip_txt))
        epis = re.findall(r"X\((\d+)\)", mac.get("GVL_A4P_EPI_LIST", (True, ""))[1])

        def expand(s):
            """textual expansion of every macro that is not a statement's text; the arguments of a function-like macro only name C++ variables and are dropped"""
            pat = re.compile(r"\b(GVL_\w+)\b(\s*\((?:[^()]|\([^()]*\))*\))?")

            def sub(m):
                n = m.group(1)
                if n not in mac or _STATEMENT.match(n):
                    return m.group(0)
                return " " + mac[n][1] + " " + ("" if mac[n][0] else (m.group(2) or ""))
            for _ in range(20):
                s2 = pat.sub(sub, s)
                if s2 == s:
                    return s
                s = s2
            raise AssertionError("macro expansion does not terminate")

        for m in re.finditer(r"asm\s+volatile\s*\(", hip_txt):
            depth, i, q = 1, m.end(), False
            while depth:
                ch = hip_txt[i]
                if ch == '"' and hip_txt[i - 1] != "\\":
                    q = not q
                elif not q:
                    depth += ch == "("
                    depth -= ch == ")"
                i += 1
            body = hip_txt[m.end():i - 1].strip()
            head = re.match(r"(GVL_\w+?)(##E)?\b", body)
            if not head or not (head.group(2) or _STATEMENT.match(head.group(1))):
                continue                                                     # a statement written out in the .hip itself (register reads of the epilogue, waits)
            for e in (epis if head.group(2) else [None]):
                txt = body if e is None else re.sub(r"E\s*##\s*E\b", f"E{e}", body)
                name = re.match(r"\w+", txt).group(0)
                assert _STATEMENT.match(name) and name in mac, f"{hip}: asm statement {name} has no generated text in {inc}"
                secs = _split_top(expand(txt[len(name):]), ":")
                assert 3 <= len(secs) <= 4 and not secs[0].strip(), (hip, name, len(secs))
                outs, inouts, _, k = _constraints(secs[1], "out", 0)
                _, _, ins, _ = _constraints(secs[2], "in", k)
                clob = set()
                for c in re.findall(r'"(\w+)"', secs[3] if len(secs) > 3 else ""):
                    if c != "memory":
                        clob |= _regs(c)
                lines = [l.replace("\\n\\t", "").strip() for l in re.findall(r'"((?:[^"\\]|\\.)*)"', mac[name][1])]
                findings += _audit_statement(name, lines, outs, inouts, ins, clob)
                seen.append(name)
    return findings, seen


def test_asm_statements_write_only_what_they_declare():
    findings, seen = audit_asm_contract()
    epis = [0, 32, 64, 128, 8, 136, 184, 98, 3, 67]
    want = {f"GVL_A4_TILE_ASM_V{v}" for v in range(3)} | {"GVL_A4_DMA_TILE_ASM", "GVL_A4P_DMA_TILE_ASM"} | {f"GVL_A4P_{k}_E{e}" for k in ("TILE0", "TILE", "FLUSH") for e in epis}
    assert set(seen) == want, f"statements not audited: {sorted(want - set(seen))}; unexpected: {sorted(set(seen) - want)}"
    assert not findings, f"{len(findings)} undeclared register uses:\n" + "\n".join(findings)


def test_the_audit_rejects_an_undeclared_write_a_stale_read_and_an_unknown_mnemonic():
    """the audit can fail: a statement that writes into its input block, one that reads a scratch register it never wrote, one that leaves m0 changed, and a mnemonic the table does not know"""
    ins = {("v", i) for i in range(16)} | {("s", 36)}
    clob = {("v", 200), ("v", 201), ("s", 72), ("scc", 0), ("vcc", 0)}
    ok = ["v_mov_b32 v200, v3", "v_cmp_eq_u32 vcc, 3, v200", "v_cndmask_b32 v201, v201, v200, vcc"]
    assert _audit_statement("t", ok[:2], set(), set(), ins, clob) == []
    f = _audit_statement("t", ["v_mov_b32 v200, v3", "v_cndmask_b32 v12, v12, v200, vcc"], set(), set(), ins | {("vcc", 0)}, clob)
    assert len(f) == 1 and "writes v12" in f[0], f
    assert _audit_statement("t", ["v_mov_b32 v200, v3", "v_cndmask_b32 v12, v12, v200, vcc"], set(), {("v", i) for i in range(16)}, {("s", 36), ("vcc", 0)}, clob) == []
    f = _audit_statement("t", ok, set(), set(), ins, clob)
    assert len(f) == 1 and "reads before any write v201" in f[0], f
    f = _audit_statement("t", ["s_add_u32 m0, s36, 0x1000", "buffer_load_dwordx4 v3, s[36:39], s72 offen lds"], set(), set(), ins | {("s", i) for i in range(36, 40)} | {("s", 72)}, clob)
    assert len(f) == 1 and "m0" in f[0], f
    assert _audit_statement("t", ["s_mov_b32 s72, m0", "s_add_u32 m0, s36, 0x1000", "s_mov_b32 m0, s72"], set(), set(), ins, clob) == []
    with pytest.raises(AssertionError, match="destination-operand table"):
        _audit_statement("t", ["v_fma_f32 v200, v1, v2, v3"], set(), set(), ins, clob)
