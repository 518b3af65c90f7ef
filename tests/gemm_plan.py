"""Which kernel form(s) a GEMM launch takes: a thin wrapper over tests/c/gemm_plan_dump.cc, i.e. over the library's own decision function
(csrc/gvl_gemm_plan.h: host-only, no GPU).  Used by tests/test_gemm_plan_cpu.py (recorded decisions) and by the GPU tests of the GEMM forms, which are bit-identical by
design: only the plan can say which kernel a case exercised."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grounded-video-llm_amd", "csrc")

# GemmForm (gvl_gemm_plan.h)
LOCKSTEP_128, T128, T64x128, PP_STAGED, PP_LANE, A4_S0, A4_S1, A4_S2, A4P = range(9)
FORM_OF_CFG = {84: A4_S0, 86: A4_S1, 87: A4_S2, 88: A4P, 22: T64x128}     # the form an explicit tile_cfg asks for
BIG_FORMS = (PP_STAGED, PP_LANE, A4_S0, A4_S1, A4_S2, A4P)                 # 256 x 256 tiles, 32-bit operand offsets
# epilogue code bits (epi_code)
QGELU, GELU, SWIGLU, F32, RESID, GAMMA, BIAS, ROWSCALE, ROWSQ = 1, 2, 3, 4, 8, 16, 32, 64, 128
STAGED = (0, 32, 33, 34, 3, 56, 8, 64, 67, 98, 128, 136, 184, 4, 36, 44)
A4_EPIS = tuple(e for e in STAGED if not e & F32)
A4P_MIN_NK = {0: 3, 32: 3, 64: 3, 128: 7, 8: 12, 136: 12, 184: 16, 98: 15, 3: 9, 67: 9}      # GVL_A4P_MIN_NK_E* (generated: csrc/gvl_gemm4p_loop.inc)


@functools.lru_cache(maxsize=None)
def dumper():
    exe = os.path.join(tempfile.mkdtemp(prefix="gvl_plan_"), "gemm_plan_dump")
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", CSRC, os.path.join(ROOT, "tests", "c", "gemm_plan_dump.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def case(M, N, K, epi=0, cfg=0, lda=-1, ldw=0, ldc=-1, ldr=-1, grp_rows=0, rowsq_ld=-1, ptr16=1, a4_mode=1, lab_cfg=0, small_pct=-1, small64=-1):
    """a full case row; -1 = what gvl_op_gemm / gvl_op_gemm_rows pass (dense operands, SwiGLU halves the output width)"""
    return [M, N, K, epi, cfg, K if lda < 0 else lda, ldw, (N // 2 if epi & 3 == SWIGLU else N) if ldc < 0 else ldc, N if ldr < 0 else ldr, grp_rows,
            (N // 64 if epi & ROWSQ else 0) if rowsq_ld < 0 else rowsq_ld, ptr16, a4_mode, lab_cfg, small_pct, small64]


def plans(cases, n_cu):
    """cases: rows as case() returns them -> per case None (the launch is refused) or (launches [(form, epi, m0, m1, n0, n1)], whole cost, chosen cost)"""
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (c[0], c[1], c[2], c[5], c[6], c[7], c[8], c[9], c[10], c[3], c[4], c[11], c[12], n_cu, c[13], c[14], c[15])
                   for c in cases)
    r = subprocess.run([dumper()], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    out = []
    for ln in lines:
        t = ln.split()
        if t[0] != "0":
            out.append(None)
            continue
        v = [int(x) for x in t[3:]]
        out.append(([tuple(v[i:i + 6]) for i in range(0, len(v), 6)], float(t[1]), float(t[2])))
    return out


def epi_of(act=0, out_f32=False, resid=None, gamma=None, bias=None, rowscale=None, want_rowsq=False, **_):
    """the epilogue code of an Engine.op_gemm / op_gemm_rows call's keyword arguments"""
    return (act & 3) | (F32 if out_f32 else 0) | (RESID if resid is not None else 0) | (GAMMA if gamma is not None else 0) | (BIAS if bias is not None else 0) | \
        (ROWSCALE if rowscale is not None else 0) | (ROWSQ if want_rowsq else 0)


@functools.lru_cache(maxsize=None)
def device_cus():
    import ctypes as C
    from grounded_video_llm_amd import lib as L
    arch, cus = C.create_string_buffer(64), C.c_int(0)
    rc = L.load().gvl_device_info(arch, 64, C.byref(cus))
    assert rc == 0, rc
    return cus.value


@functools.lru_cache(maxsize=None)
def forms(M, N, K, epi, cfg):
    """the forms that Engine.op_gemm / op_gemm_rows (M, N, K, epilogue, tile_cfg) runs on this device, in launch order"""
    p = plans([case(M, N, K, epi, cfg)], device_cus())[0]
    assert p is not None, f"{M}x{N}x{K} epilogue {epi} tile_cfg {cfg}: refused"
    return tuple(l[0] for l in p[0])


def assert_runs(form, M, N, K, cfg, **kw):
    got = forms(M, N, K, epi_of(**kw), cfg)
    assert form in got, f"{M}x{N}x{K} epilogue {epi_of(**kw)} tile_cfg {cfg}: the plan is forms {got}, not form {form} -- this case does not exercise the kernel it is about"
