"""CPU tests of the product's host-side logic (no GPU): prompt/integer plumbing against the reference-generated
goldens, the weight packer's layout transforms against the oracle's un-fused maths, and the C ABI surface."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gvl_oracle as O
from conftest import GOLDEN, ROOT
from grounded_video_llm_amd import lib as L, prompts as P, synth, weights as Wt


def test_prompts_against_reference_goldens():
    g = json.load(open(os.path.join(GOLDEN, "integer_paths.json")))
    for k, v in g["frame_indices"].items():
        n, vlen = map(int, k.split("_"))
        assert P.sample_frame_indices(n, vlen) == v, k
    for k, v in g["prompts"].items():
        llm, mode = k.split("|")
        assert P.build_prompt(llm, mode, g["prompt_text"]) == v, k
    for k, v in g["parse_time_interval"].items():
        llm, txt, dur = k.split("|")
        assert P.parse_time_interval(txt, float(dur), 300, llm) == v, k
    for k, v in g["tokenizer_image_token"].items():
        name, pr = k.split("|", 1)
        def tok(s, nb=(name == "nobos")):
            ids = [3 + (sum(map(ord, w)) % 90) for w in s.split()]
            return ids if nb else [1] + ids
        assert P.tokenize_with_image(pr, tok, 1) == v, k
    assert P.spatial_indices(96, 12) == [4 + 8 * i for i in range(12)]
    assert P.seconds_to_tokens("What is happening from 70 seconds to 80 seconds?", 118.3) == "What is happening from <177> to <202>?"
    assert P.parse_time_interval("From <36> to <64>.", 118.3) == "From  14.20 seconds to  25.24 seconds."
    assert len(P.temporal_token_strings(300)) == 302
    # referring prompt == oracle's
    q = "What is happening from 70 seconds to 80 seconds?"
    assert P.build_prompt("phi3.5", "referring", q, 118.3) == O.build_prompt("phi3.5", "referring", q, 118.3)
    with pytest.raises(ValueError):
        P.parse_time_interval("<3>", 10.0, 300, "vicuna")


def test_left_pad_truncate_matches_oracle():
    rng = np.random.default_rng(1)
    for _ in range(20):
        batch = [rng.integers(3, 90, size=int(rng.integers(1, 30))).tolist() for _ in range(int(rng.integers(1, 4)))]
        mx = int(rng.integers(4, 40))
        a, am = P.left_pad_truncate(batch, 0, mx)
        b, bm = O.left_pad_truncate(batch, 0, mx)
        assert np.array_equal(a, b.numpy()) and np.array_equal(am, bm.numpy())


def test_packer_fusions_are_exact():
    # CLIP qkv fuse, Phi gate/up interleave, Llama q/k/v + gate/up fuse, LoRA merge, K padding, pos-embed interpolation
    Wc = synth.clip_weights(64, 128, 2, 28, 14, seed="t.pack.clip")
    pc = Wt.pack_clip(Wc, 1)
    assert pc["clip.patch.w"].shape == (64, 640) and float(pc["clip.patch.w"][:, 588:].abs().max()) == 0.0
    q = Wc["vision_model.encoder.layers.0.self_attn.q_proj.weight"].to(torch.bfloat16)
    assert torch.equal(pc["clip.L0.qkv.w"][:64], q)
    Wl = synth.llm_weights("phi3", 64, 128, 1, 4, 4, 50, True, seed="t.pack.phi")
    pl = Wt.pack_llm(Wl, "phi3", 1, 4, 4, 128, 10000.0, *synth.longrope_factors(16))
    gu = Wl["model.layers.0.mlp.gate_up_proj.weight"].to(torch.bfloat16)
    assert torch.equal(pl["llm.L0.gu.w"][0::2], gu[:128]) and torch.equal(pl["llm.L0.gu.w"][1::2], gu[128:])
    assert pl["rope.cos_s"].shape == (128, 8) and "rope.cos_l" in pl
    ocfg = O.LLMConfig("phi3", 64, 128, 1, 4, 4, 50, 1e-5, 10000.0, 131072, 4096, *synth.longrope_factors(16))
    cos, sin = O.rope_cos_sin(ocfg, torch.arange(128), 128, emu=True)
    assert torch.equal(pl["rope.cos_s"], cos[:, :8]) and torch.equal(pl["rope.sin_s"], sin[:, :8])
    cosl, _ = O.rope_cos_sin(ocfg, torch.arange(128), 5000, emu=True)
    assert torch.equal(pl["rope.cos_l"], cosl[:, :8])
    Wm = synth.llm_weights("llama", 64, 128, 1, 4, 2, 50, True, seed="t.pack.llama")
    pm = Wt.pack_llm(Wm, "llama", 1, 4, 2, 64, 500000.0)
    assert pm["llm.L0.qkv.w"].shape == (64 + 32 + 32, 64) and "rope.cos_l" not in pm
    # LoRA: peft-style keys merged == oracle's un-merged maths
    A, B = synth.det_tensor("t.lora.A", (8, 64), 0.1), synth.det_tensor("t.lora.B", (192, 8), 0.1)
    Wp = {("base_model.model." + k): v for k, v in Wl.items()}
    Wp["base_model.model.model.layers.0.self_attn.qkv_proj.lora_A.default.weight"] = A
    Wp["base_model.model.model.layers.0.self_attn.qkv_proj.lora_B.default.weight"] = B
    pp = Wt.pack_llm(Wp, "phi3", 1, 4, 4, 128, 10000.0, lora_alpha=16.0, lora_r=8)
    want = O.lora_merge(Wl["model.layers.0.self_attn.qkv_proj.weight"], A, B, 16.0, 8).to(torch.bfloat16)
    assert torch.equal(pp["llm.L0.qkv.w"], want)
    # pos-embed interpolation == oracle == reference golden
    z = np.load(os.path.join(GOLDEN, "iv2_pos_interp.npz"))
    meta = json.loads(str(z["meta"]))
    src = synth.det_tensor(meta["src"], meta["src_shape"])
    np.testing.assert_allclose(Wt.interpolate_pos_embed_t(src, 4, 8).numpy(), z["pos"], atol=1e-6)


def test_c_abi_exports_every_declared_symbol():
    """libgvl.so must load (no GPU needed) and export exactly what include/gvl.h declares."""
    hdr = open(os.path.join(ROOT, "include", "gvl.h")).read()
    declared = sorted(set(re.findall(r"\b(gvl_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 20
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in gvl.h but not exported"
    assert sorted(L.EXPORTS) == declared, "lib.py binds a different set of symbols than gvl.h declares"
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r" T (gvl_[a-z_0-9]+)", out)))
    assert exported == declared
    # the struct layout the Python side uses matches the header's field count
    n_fields = len(re.findall(r"^\s*(?:int32_t|float)\s+[^;]+;", hdr.split("typedef struct {")[1].split("} gvl_config;")[0], re.M))
    assert n_fields >= 10 and ctypes.sizeof(L.GvlConfig) == 4 * len(L.GvlConfig._fields_)


def test_seq_pages_accessor_without_a_ctx_is_an_argument_error_that_writes_nothing():
    """gvl_debug_seq_pages is host-only: it can be called here.  Its argument handling on a live table is SeqTable::pages_of's (test_seq_table_cpu.py); what the entry
    adds is the ctx check"""
    lib = L.load()
    buf, n = (ctypes.c_int32 * 4)(-7, -7, -7, -7), ctypes.c_int(-9)
    assert lib.gvl_debug_seq_pages(None, 0, buf, 4, ctypes.byref(n)) == L.ERR_ARG == lib.gvl_debug_seq_pages(None, 0, None, 0, None)
    assert list(buf) == [-7] * 4 and n.value == -9


def test_product_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = L.load()
    cfg = L.GvlConfig()
    h = ctypes.c_void_p()
    rc = lib.gvl_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -5 and b"no CPU fallback" in lib.gvl_last_error(None)
    from grounded_video_llm_amd import engine as E
    with pytest.raises(RuntimeError):
        E.Engine(E.TowerGeometry(), "cpu")


def test_rccl_missing_is_an_error_not_a_crash():
    """A host without librccl: gvl_comm_unique_id must return GVL_ERR_STATE with a message (include/gvl.h), not crash the process.
    GVL_RCCL_LIB points the loader at a file that does not exist; own process because the loader caches its first attempt."""
    code = (
        "import ctypes, sys\n"
        f"lib = ctypes.CDLL({L.LIB_PATH!r})\n"
        "lib.gvl_last_error.restype = ctypes.c_char_p; lib.gvl_last_error.argtypes = [ctypes.c_void_p]\n"
        "buf = ctypes.create_string_buffer(128)\n"
        "rc = lib.gvl_comm_unique_id(buf)\n"
        "rc2 = lib.gvl_comm_unique_id(buf)\n"
        "print(rc, rc2, lib.gvl_last_error(None).decode())\n")
    env = dict(os.environ, GVL_RCCL_LIB="/nonexistent/librccl-missing.so")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f"process died: rc {r.returncode} {r.stderr[-500:]}"
    rc, rc2, msg = r.stdout.strip().split(" ", 2)
    assert rc == "-2" and rc2 == "-2" and "dlopen(librccl) failed" in msg and "librccl-missing" in msg


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "grounded-video-llm_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "gvl_oracle" not in src and "oracle/" not in src.replace("the oracle", ""), f"{f} references the oracle"


@pytest.mark.parametrize("llm", ["phi3.5", "llama3"])
def test_reference_checkpoint_layout_roundtrip(tmp_path, llm):
    """SURVEY §8 f3 (real-checkpoint tooling): a directory laid out like the reference's weights (models/llava_next_video.py:117-151:
    vision_model.pth, image_newline(s).pth, multi_modal_projector.pth, language_model_seperated/*.safetensors, InternVideo2 .pt) plus an
    inference.py-style fine-tuned ckpt overlay (:156-162) must load and pack to exactly the tensors the in-memory state dicts give."""
    from safetensors.torch import save_file
    from grounded_video_llm_amd import model as M, synth, weights as Wt
    kind = "phi3" if llm == "phi3.5" else "llama"
    hid, vocab, kvh = 64, 128, 4 if llm == "phi3.5" else 2
    sd = {"vision_tower": synth.clip_weights(64, 128, 3, seed="ck.clip"), "video_encoder": synth.iv2_weights(64, 128, 3, 2, seed="ck.iv2"),
          "projectors": synth.projector_weights(llm, hid, 64, 64, seed="ck.proj"),
          "language_model": synth.llm_weights(kind, hid, 128, 2, 4, kvh, vocab, True, seed="ck.llm")}
    d = tmp_path / "Phi-3.5-vision-instruct-seperated"
    (d / "language_model_seperated").mkdir(parents=True)
    torch.save(sd["vision_tower"], d / "vision_model.pth")
    torch.save({k.split(".", 1)[1]: v for k, v in sd["projectors"].items() if k.startswith("multi_modal_projector.")}, d / "multi_modal_projector.pth")
    if llm == "phi3.5":
        torch.save({"glb_GN": sd["projectors"]["glb_GN"], "sub_GN": sd["projectors"]["sub_GN"]}, d / "image_newlines.pth")
    else:
        torch.save({"image_newline": sd["projectors"]["image_newline"]}, d / "image_newline.pth")
    lm = {k: v.contiguous() for k, v in sd["language_model"].items()}
    keys = sorted(lm)
    save_file({k: lm[k] for k in keys[: len(keys) // 2]}, str(d / "language_model_seperated" / "model-00001-of-00002.safetensors"))
    save_file({k: lm[k] for k in keys[len(keys) // 2:]}, str(d / "language_model_seperated" / "model-00002-of-00002.safetensors"))
    iv2_path = tmp_path / "vision-encoder-InternVideo2.pt"
    torch.save(sd["video_encoder"], iv2_path)
    base = M.load_reference_checkpoints(llm, str(iv2_path), str(d))
    # the video projector is a trained group: absent from the base directory (zeros until the fine-tuned ckpt arrives, inference.py:159-160)
    assert torch.count_nonzero(base["projectors"]["video_projecter.up_proj.weight"]) == 0
    ckpt = {"video_projecter": {k.split(".", 1)[1]: v for k, v in sd["projectors"].items() if k.startswith("video_projecter.")},
            "multi_modal_projector": {k.split(".", 1)[1]: v for k, v in sd["projectors"].items() if k.startswith("multi_modal_projector.")}}
    proj = dict(base["projectors"])
    for grp in ("multi_modal_projector", "video_projecter"):
        for k, v in ckpt[grp].items():
            proj[f"{grp}.{k}"] = v
    for name, a, b in (("clip", Wt.pack_clip(base["vision_tower"], 2), Wt.pack_clip(sd["vision_tower"], 2)),
                       ("iv2", Wt.pack_iv2(base["video_encoder"], 2, 2), Wt.pack_iv2(sd["video_encoder"], 2, 2)),
                       ("proj", Wt.pack_projectors(proj, llm), Wt.pack_projectors(sd["projectors"], llm)),
                       ("llm", Wt.pack_llm(base["language_model"], kind, 2, 4, kvh, 256, 10000.0, None, None),
                        Wt.pack_llm(sd["language_model"], kind, 2, 4, kvh, 256, 10000.0, None, None))):
        assert set(a) == set(b), name
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{name}:{k}"
    with pytest.raises(FileNotFoundError):
        M.load_reference_checkpoints(llm, str(tmp_path / "missing.pt"), str(d))
    # offline packing CLI: reference directory (+ fine-tuned ckpt) -> ONE packed file -> exactly the tensors of the in-memory path
    import importlib.util
    spec = importlib.util.spec_from_file_location("pack_checkpoint", os.path.join(ROOT, "tools", "pack_checkpoint.py"))
    pc = importlib.util.module_from_spec(spec); spec.loader.exec_module(pc)
    from grounded_video_llm_amd.engine import TowerGeometry
    geo = TowerGeometry(llm=llm, clip_hidden=64, clip_inter=128, clip_layers=3, clip_heads=4, iv2_dim=64, iv2_inter=128, iv2_depth=3, iv2_heads=4,
                        hidden=hid, inter=128, layers=2, heads=4, kv_heads=kvh, vocab=vocab, max_seq=256, rope_orig_max_pos=0)
    ck_path = tmp_path / "sft.pth"
    torch.save({"model": ckpt}, ck_path)
    out = tmp_path / "w.gvl.safetensors"
    pc.main(["--llm", llm, "--pretrained_video_path", str(iv2_path), "--pretrained_vision_proj_llm_path", str(d), "--ckpt_path", str(ck_path),
             "--num_frames", "4", "--num_segs", "2", "--out", str(out)], geometry=geo)
    got = Wt.load_packed_file(str(out))
    fitted = M.fit_geometry(geo, llm, 4, 2, 2048)      # what the CLI (and later the model constructor) derives from frames / segments / max_txt_len
    assert geo.max_seq == 256 and geo.frames_per_seg == 8, "fit_geometry must not edit the caller's object"
    assert fitted.max_seq >= 2 * (fitted.frames_per_seg * 16 + 65) + 2048 and fitted.frames_per_seg == 2
    want = pc.pack_all({**sd, "projectors": dict(sd["projectors"])}, fitted, llm)
    meta = M.packed_file_metadata(str(out))
    assert meta["max_seq"] == str(fitted.max_seq) and meta["frames_per_seg"] == "2" and meta["llm"] == llm
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k].cpu()), k
    with pytest.raises(ValueError):
        save_file({"x": torch.zeros(1)}, str(tmp_path / "other.safetensors"))
        Wt.load_packed_file(str(tmp_path / "other.safetensors"))


def test_fit_geometry_kv_pool_policy():
    """the constructor must not silently swap an explicit small KV pool for "all of the free HBM", nor edit the caller's geometry."""
    from grounded_video_llm_amd import model as M
    from grounded_video_llm_amd.engine import TowerGeometry
    g = TowerGeometry(kv_pages=80)                                  # 5120 tokens < 12 x 285 + 2048 + 256
    with pytest.raises(ValueError, match="kv_pages = 80"):
        M.fit_geometry(g, "phi3.5", 96, 12, 2048)
    assert g.kv_pages == 80 and g.max_prefill == 4096
    ok = M.fit_geometry(g, "phi3.5", 96, 12, 1024)                  # 3420 + 1024 + 256 = 4700 tokens fit
    assert ok.kv_pages == 80 and ok.max_prefill >= 4444 and ok is not g
    assert M.fit_geometry(TowerGeometry(), "phi3.5", 96, 12, 2048).kv_pages == 128      # the default pool holds the default configuration
    auto = M.fit_geometry(TowerGeometry.llama3_8b(), "llama3", 256, 32, 2048)           # 32 x 193 + 2048 + 256 > 8192 tokens: default pool -> sized from the free HBM
    assert auto.kv_pages == 0 and auto.max_seq >= 8480
    assert M.fit_geometry(TowerGeometry(kv_pages=0), "llama3", 256, 32, 2048).kv_pages == 0


# ---- continuous-batching scheduler on a scripted engine ------------------------------------------------
class _Emb:
    def __init__(self, S, seed):
        self.shape, self.seed = (S, 8), seed


class _ScriptedEngine:
    """Engine double: token t of a request is a pure function of (its seed, t); KV pages are a finite pool."""

    def __init__(self, pages, vocab=50, max_seq=4096):
        from types import SimpleNamespace
        self.free, self.vocab, self.geo = pages, vocab, SimpleNamespace(max_seq=max_seq)
        self.seqs, self.log, self._next = {}, [], 0

    def _tok(self, seed, t):
        import zlib
        return zlib.crc32(f"{seed}:{t}".encode()) % self.vocab

    def seq_alloc(self, max_tokens):
        need = (max_tokens + 63) // 64
        if need > self.free:
            e = L.GvlError("KV pages exhausted")
            e.status = L.ERR_OOM
            raise e
        self.free -= need
        self._next += 1
        self.seqs[self._next] = dict(pages=need, cap=max_tokens, seed=None, pos=0, out=[])
        return self._next

    def seq_free(self, seq):
        self.free += self.seqs.pop(seq)["pages"]

    def prefill_batch(self, seqs, embs):
        self.log.append(("prefill", [e.shape[0] for e in embs]))
        for s, e in zip(seqs, embs):
            q = self.seqs[s]
            assert q["seed"] is None and e.shape[0] <= q["cap"]
            q["seed"], q["pos"] = e.seed, e.shape[0]
            q["out"].append(self._tok(e.seed, 0))

    def decode_steps(self, seqs, k):
        assert len(set(seqs)) == len(seqs) and k >= 1
        self.log.append(("decode", len(seqs), k))
        for s in seqs:
            q = self.seqs[s]
            assert q["pos"] + k <= q["cap"], "scheduler overran a sequence's KV capacity"
            for _ in range(k):
                q["out"].append(self._tok(q["seed"], len(q["out"])))
            q["pos"] += k

    def seq_read(self, seq, first=0, cap=4096):
        return self.seqs[seq]["out"][first:first + cap]

    def alone(self, emb, max_new, eos):
        out = []
        for t in range(min(max_new, self.geo.max_seq - emb.shape[0] + 1)):
            out.append(self._tok(emb.seed, t))
            if eos is not None and out[-1] == eos:
                break
        return out


@pytest.mark.parametrize("max_active,chunk,pages", [(1, 1, 64), (4, 8, 64), (3, 5, 7), (8, 16, 1000)])
def test_scheduler_ids_equal_one_at_a_time(max_active, chunk, pages):
    from grounded_video_llm_amd import serve
    eng = _ScriptedEngine(pages)
    rng = np.random.default_rng(max_active * 100 + chunk)
    embs = [_Emb(int(rng.integers(1, 200)), int(rng.integers(1, 10**6))) for _ in range(23)]
    eos, max_new = 7, 40
    want = [eng.alone(e, max_new, eos) for e in embs]
    assert any(len(w) < max_new for w in want) and any(len(w) == max_new for w in want)      # both exits are exercised
    sch = serve.ClipScheduler(eng, eos, max_active=max_active, chunk=chunk)
    rids = [sch.submit(e, max_new) for e in embs]
    out = sch.run()
    assert [out[r] for r in rids] == want
    assert eng.free == pages and not eng.seqs, "pages leaked"
    assert sch.stats["max_concurrent"] <= max_active
    if max_active > 1 and pages >= 64:
        assert sch.stats["max_concurrent"] > 1 and any(op[0] == "prefill" and len(op[1]) > 1 for op in eng.log)
    # no decode chunk ran past a member's max_new; wasted steps (after an eos inside a chunk) are bounded by chunk - 1 per request
    assert sch.stats["wasted_seq_steps"] <= (chunk - 1) * len(embs)


def test_scheduler_edge_cases():
    from grounded_video_llm_amd import serve
    eng = _ScriptedEngine(4, max_seq=128)
    # request that cannot ever fit the KV pool -> loud error, not a spin
    sch = serve.ClipScheduler(eng, None, max_active=2, chunk=4)
    sch.submit(_Emb(100, 1), 1000)            # clamped to max_seq = 128 tokens -> 2 pages: fits
    out = sch.run()
    assert len(out[0]) == 128 - 100 + 1       # generate() stops at the context limit
    big = _ScriptedEngine(1, max_seq=4096)
    sch = serve.ClipScheduler(big, None, max_active=2, chunk=4)
    sch.submit(_Emb(100, 1), 100)             # 200 tokens = 4 pages > pool of 1
    with pytest.raises(L.GvlError, match="does not fit"):
        sch.run()
    # eos as the very first (prefill) token and max_new == 1: finish without a decode step
    eng = _ScriptedEngine(16)
    e = _Emb(10, 5)
    first = eng._tok(5, 0)
    assert serve.generate_many(eng, [e, _Emb(12, 6)], 1, None) == [[first], [eng._tok(6, 0)]]
    assert serve.generate_many(eng, [e], 9, first) == [[first]]
    assert not any(op[0] == "decode" for op in eng.log)
    # prefill workspace limit: newcomers are split over iterations
    eng = _ScriptedEngine(64)
    out = serve.generate_many(eng, [_Emb(60, i) for i in range(4)], 3, None, max_active=4, chunk=2, max_prefill_rows=128)
    assert [op[1] for op in eng.log if op[0] == "prefill"][:2] == [[60, 60], [60, 60]] and len(out) == 4
    with pytest.raises(ValueError):
        serve.ClipScheduler(eng, None, max_active=0)


def test_header_is_plain_c_and_links(tmp_path):
    """include/gvl.h compiles as strict C99 (nothing but <stdint.h>), a C program links libgvl.so and -- on a host without a GPU --
    gets GVL_ERR_NOGPU from gvl_create: the boundary is a C ABI, not a Python extension."""
    L.load()                                                  # builds the library if needed
    exe = str(tmp_path / "abi_consumer")
    libdir = os.path.dirname(L.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "abi_consumer.c"), "-o", exe, "-L", libdir, "-lgvl", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    if not torch.cuda.is_available():
        assert "create=-5" in r.stdout and "no CPU fallback" in r.stdout


def test_host_integer_paths_fuzz_against_oracle():
    """The product's host-side integer / text plumbing (prompts.py) against the oracle restatement (pinned on the reference's own
    outputs) on random inputs: frame sampling, temporal-token <-> seconds, <image> splitting, padding, conversation templates,
    training label masks -- all bit-exact."""
    rng = np.random.default_rng(7)
    words = ["the", "door", "opens", "<image>", "a", "person", "walks", "<17>", "<timestamp_grounding>", "?", "video", "12 seconds", "from", "to", "<300>", "3 seconds"]
    tok = lambda s: [1] + [3 + (sum(map(ord, w)) % 90) for w in s.split()]
    tok_nobos = lambda s: [3 + (sum(map(ord, w)) % 90) for w in s.split()]
    for _ in range(300):
        nf, vlen = int(rng.integers(1, 300)), int(rng.integers(1, 9000))
        assert P.sample_frame_indices(nf, vlen) == O.get_frame_indices(nf, vlen)
        segs = int(rng.integers(1, 33)); nfr = segs * int(rng.integers(1, 17))
        assert P.spatial_indices(nfr, segs) == O.spatial_frame_indices(nfr, segs)
        dur, t = float(rng.uniform(0.5, 4000)), float(rng.uniform(0, 4000))
        assert P.quantize_time(min(t, dur), dur, 300) == O.quantize_timestamp(min(t, dur), dur, 300)
        text = " ".join(rng.choice(words, size=int(rng.integers(1, 14))))
        assert P.seconds_to_tokens(text, dur) == O.seconds_to_temporal_tokens(text, dur)
        for llm in ("phi3.5", "llama3"):
            assert P.parse_time_interval(text, dur, 300, llm) == O.parse_time_interval(text, dur, 300, llm)
        for tk, bos in ((tok, 1), (tok_nobos, 1), (tok, None)):
            assert P.tokenize_with_image(text, tk, bos) == O.tokenizer_image_token(text, tk, bos)
    for _ in range(60):
        rows = [list(rng.integers(3, 90, size=int(rng.integers(1, 40)))) for _ in range(int(rng.integers(1, 6)))]
        mtl = int(rng.integers(1, 50))
        a_ids, a_mask = P.left_pad_truncate(rows, 0, mtl)
        o_ids, o_mask = O.left_pad_truncate(rows, 0, mtl)
        assert np.array_equal(a_ids, o_ids.numpy()) and np.array_equal(a_mask, o_mask.numpy())
    # conversations: templates + label masks, 1-4 rounds, image token in the first question, all three LLM families
    for _ in range(120):
        llm = ("phi3.5", "llama3", "vicuna")[int(rng.integers(0, 3))]
        conv = []
        for r in range(int(rng.integers(1, 5))):
            q = " ".join(rng.choice(words[:3] + words[4:7] + ["?"], size=int(rng.integers(1, 8))))
            a = " ".join(rng.choice(words[:3] + words[4:8] + ["."], size=int(rng.integers(0, 8))))
            conv += [{"from": "human", "value": ("<image>\n" if r == 0 else "") + q}, {"from": "gpt", "value": a}]
        text = P.TEMPLATES[llm].encode(conv)
        assert text == O.template_encode(llm, conv)
        mtl = int(rng.integers(20, 400))
        pad = int(rng.choice([0, 2]))
        try:
            o = O.prepare_batch(llm, [text], tok, 1, pad, 2, mtl)
        except Exception as e:
            with pytest.raises(type(e)):
                P.prepare_batch(llm, [text], tok, 1, pad, 2, mtl)
            continue
        p = P.prepare_batch(llm, [text], tok, 1, pad, 2, mtl)
        for x, y in zip(p, o):
            assert np.array_equal(x, y.numpy()), (llm, text)


# ---- round-2 loader fixes: real-checkpoint shaped inputs that the synthetic round trip above never exercised ------
def test_exact_tensor_matches_a_numpy_uint64_restatement():
    """synth.exact_tensor is what lets the reference (CPU, build container) and the HIP path (GPU) consume the SAME full-size weights
    without a fixture: integer hashing + two IEEE f32 ops.  Checked here against an independent numpy uint64 implementation; the
    GPU == CPU half is tests/test_gpu_c0.py::test_exact_tensor_is_bit_identical_on_the_gpu."""
    from grounded_video_llm_amd import synth

    def ref(name, n, std, mean):
        s = synth._seed_of(name); s0 = np.uint64(s & 0xFFFFFFFF); s1 = np.uint64((s >> 32) & 0xFFFFFFFF); M = np.uint64(0xFFFFFFFF)

        def f(x):
            x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x85EBCA6B)) & M; x = x ^ (x >> np.uint64(13)); x = (x * np.uint64(0xC2B2AE35)) & M
            return x ^ (x >> np.uint64(16))
        h = f(np.arange(n, dtype=np.uint64) ^ s0); h = f((h + s1) & M)
        u = (h >> np.uint64(8)).astype(np.float32) * np.float32(1 / 16777216.0) - np.float32(0.5)
        u = u * np.float32(2 * np.sqrt(3.0) * std)
        return u + np.float32(mean) if mean != 0 else u
    for name, shape, std, mean in (("a/b", (257, 33), 0.02, 0.0), ("norm", (1000,), 0.1, 1.0), ("c0.llm/embed", (5, 3072), 0.5, 0.0)):
        x = synth.exact_tensor(name, shape, std, mean, chunk=1000)
        assert np.array_equal(x.numpy().ravel(), ref(name, int(np.prod(shape)), std, mean))
        assert abs(float(x.std()) - std) < 0.1 * std


def test_iv2_f4_checkpoint_is_interpolated_to_frames_per_seg():
    """The released InternVideo2 checkpoint is `-f4` (pos_embed 1 + 4*L rows); the reference interpolates it to frames_per_seg at load
    (interpolate_pos_embed_internvideo2_new(..., orig_t_size=4), models/llava_next_video.py:131 -> internvideo2.py:260-320).  pack_iv2
    must do that WITHOUT being told the checkpoint's temporal size -- golden: tests/golden/iv2_pos_interp.npz from the reference."""
    from grounded_video_llm_amd import synth, weights as Wt
    z = np.load(os.path.join(GOLDEN, "iv2_pos_interp.npz"))
    meta = json.loads(str(z["meta"]))
    W = synth.iv2_weights(64, 128, 3, 4, 28, 14, seed="f4")                  # a 4-frame checkpoint, L = 4 tokens per frame
    W["pos_embed"] = synth.det_tensor(meta["src"], meta["src_shape"])
    for kw in ({"tokens_per_frame": 4}, {}):                                   # with the grid known, and inferred (square grid, t = 4)
        got = Wt.pack_iv2(W, 2, 8, **kw)["iv2.pos"]
        assert got.shape == (1 + 8 * 4, 64)
        assert torch.equal(got, torch.from_numpy(z["pos"]).reshape(-1, 64).to(torch.bfloat16))
    assert Wt.iv2_ckpt_frames(1 + 4 * 256, 8) == 4 and Wt.iv2_ckpt_frames(1 + 8 * 256, 8) == 8 and Wt.iv2_ckpt_frames(1 + 4 * 256, 8, 256) == 4
    with pytest.raises(ValueError):
        Wt.iv2_ckpt_frames(1 + 7 * 250, 8)


def test_phi35_geometry_reads_longrope_from_config_json_and_refuses_without(tmp_path):
    """Phi3LongRoPEScaledRotaryEmbedding applies short_factor and the sqrt(1 + ln(s)/ln(orig)) scale at EVERY length
    (modeling_phi3.py:380-409): a Phi-3.5 model built without the factors of config.json would silently run plain RoPE."""
    from grounded_video_llm_amd import model as M, weights as Wt
    from grounded_video_llm_amd.engine import TowerGeometry
    short = [1.0 + 0.01 * i for i in range(48)]
    long = [1.0 + 1.5 * i for i in range(48)]
    d = tmp_path / "sep" / "language_model_seperated"
    d.mkdir(parents=True)
    cfg = {"hidden_size": 3072, "intermediate_size": 8192, "num_hidden_layers": 32, "num_attention_heads": 32, "num_key_value_heads": 32,
           "rms_norm_eps": 1e-05, "rope_theta": 10000.0, "max_position_embeddings": 131072, "original_max_position_embeddings": 4096,
           "rope_scaling": {"type": "su", "short_factor": short, "long_factor": long}}
    (d / "config.json").write_text(json.dumps(cfg))
    geo = M.geometry_from_checkpoint_dirs("phi3.5", None, str(tmp_path / "sep"))
    assert geo.vocab == 32064 + 302 and geo.lm_head_bias                                       # stage sft: reset_embeddings ran (:153-154)
    g_pre = M.geometry_from_checkpoint_dirs("phi3.5", None, str(tmp_path / "sep"), stage="pretrain")
    assert g_pre.vocab == 32064 and not g_pre.lm_head_bias                                      # stage pretrain: base vocabulary, bias-free lm_head
    assert M.geometry_from_checkpoint_dirs("llama3", None, None, "grounded", 300).vocab == 128558
    assert geo.rope_short == short and geo.rope_long == long and geo.rope_max_pos == 131072 and geo.rope_orig_max_pos == 4096
    # the tables built from that geometry carry the short factors and the 1.19 scale even at position 1 (i.e. below 4096)
    cs, sn = Wt.rope_tables(96, 8, geo.rope_theta, geo.rope_short, geo.rope_max_pos, geo.rope_orig_max_pos)
    plain_c, _ = Wt.rope_tables(96, 8, geo.rope_theta, None, geo.rope_max_pos, geo.rope_orig_max_pos)
    sf = (1 + np.log(32) / np.log(4096)) ** 0.5
    assert abs(float(cs[0, 0]) - float(torch.tensor(sf).bfloat16())) < 1e-6 and abs(float(plain_c[0, 0]) - 1.0) < 1e-6
    assert not torch.equal(cs[5], plain_c[5])
    # no config.json anywhere -> the constructor refuses (before touching the GPU) instead of running plain RoPE
    with pytest.raises(ValueError, match="LongRoPE"):
        M.LLAVA_NEXT_VIDEO(llm="phi3.5", stage="sft", config_path=str(tmp_path / "nothing"), pretrained_vision_proj_llm_path=str(tmp_path / "nothing"),
                           tokenizer=M.SyntheticTokenizer(32366))
    with pytest.raises(ValueError):
        TowerGeometry().apply_hf_config({"rope_scaling": {"type": "linear", "factor": 2.0}})
    # prompts up to max_txt_len must fit the prefill workspace (12 x 285 visual rows + 2048 text tokens > the old 4096 cap)
    g2 = TowerGeometry().apply_hf_config(cfg)
    g2.max_prefill = 2048
    gf = M.fit_geometry(g2, "phi3.5", 96, 12, 2048)      # what the constructor does first -- on a copy
    assert g2.max_prefill == 2048
    g2 = gf
    assert g2.max_prefill >= 12 * 285 + 2048 and g2.max_seq >= g2.max_prefill and g2.kv_pages * 64 >= g2.max_prefill + 256
    assert geo.kv_pages == 0                  # geometry built from the checkpoint directories: KV pool sized from the free HBM


def test_reset_embeddings_grows_a_base_language_model():
    """models/llava_next_video.py:231-268: +302 rows filled with the mean row for embed_tokens and lm_head, and an lm_head bias."""
    from grounded_video_llm_amd import synth, weights as Wt
    W = synth.llm_weights("phi3", 64, 128, 1, 4, 4, 100, lm_head_bias=False, seed="re")
    G = Wt.reset_embeddings(W, 302, True)
    for k in ("model.embed_tokens.weight", "lm_head.weight"):
        assert G[k].shape == (402, 64) and torch.equal(G[k][:100], W[k])
        assert torch.allclose(G[k][100:], W[k].mean(0, keepdim=True).expand(302, -1), atol=1e-7)
    assert G["lm_head.bias"].shape == (402,) and "lm_head.bias" not in W
    packed = Wt.pack_llm(G, "phi3", 1, 4, 4, 64, 10000.0)
    assert packed["llm.embed"].shape == (402, 64) and packed["llm.head.b"].shape == (402,)


def test_committed_bench_line_meets_the_driver_contract():
    """The one JSON line bench.py prints (committed copy of a default run: profiles/rNN_bench_1gpu.json, newest round) carries every field the driver
    and the tier's measurement rules ask for, with consistent values."""
    import glob
    path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench_1gpu.json")))[-1]       # the newest round's committed line
    d = json.loads(open(path).read().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "clips/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert "workload" in d["config"] and "model" not in d["config"]
    cps = d["config"]["clips_per_step"]
    assert abs(d["value"] - d["n_gpus"] * cps / (d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]       # value == whole-job clips / measured time
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["peak"] == 2500.0
    assert r["traffic"] is None or "traffic_source" in r
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["oracle_ids_equal_reference_golden"] is True
    if "r03" in path or "r04" in path or "r05" in path:
        # round 3: the north-star sharded single-clip latency, honest key names, the profiled pass = the timed step's launches
        assert d["single_clip_latency_ms_sharded"] > 0 and d["ids_match_serial"] is True
        assert r["clips_in_profiled_pass"] == cps and "one_clip_serial" in r and not any(k.endswith("_per_step") for k in d["stages"])
        assert abs(d["stages"]["gemm_ms_per_clip"] - r["gemm_ms_per_clip"]) < 1e-6
        assert "ragged" in d["config"]["workload"] and d["config"]["distinct_clips_resident"] >= 2 * cps


def test_generate_kwargs_map_to_hf_token_selection_semantics():
    """generate(**kw) -> token selection (the reference forwards do_sample / num_beams / temperature / top_p to HF generate,
    inference.py:170-176 -> models/llava_next_video.py:655-661): greedy unless do_sample; HF's defaults temperature 1.0 and top_k 50 when
    not given; HF's argument checks; an unseeded call takes its seed from torch's CPU generator (so torch.manual_seed governs it)."""
    from grounded_video_llm_amd.call import resolve_call

    def sel(**kw):
        c = resolve_call(kw, entry="generate", n_samples=1, eos_id=2, pad_id=0, vocab=640, draw_seed=lambda: int(torch.randint(0, 2 ** 62, (1,)).item()))
        return c.sampling_args, c.warpers                  # Engine.set_sampling's positional and keyword arguments
    assert sel(do_sample=False, num_beams=1, temperature=0.2, top_p=None) == ((False,), {})
    assert sel() == ((False,), {})                                   # no kwargs at all: greedy
    assert sel(do_sample=True, temperature=0.2, top_p=None, seed=7) == ((True, 0.2, 50, None, 7), {})         # the reference CLI's defaults
    assert sel(do_sample=True, seed=1) == ((True, 1.0, 50, None, 1), {})
    assert sel(do_sample=True, temperature=0.7, top_k=None, top_p=0.9, seed=3) == ((True, 0.7, 0, 0.9, 3), {})
    torch.manual_seed(123); s1 = sel(do_sample=True)[0][4]
    torch.manual_seed(123); s2 = sel(do_sample=True)[0][4]
    s3 = sel(do_sample=True)[0][4]
    assert s1 == s2 and s3 != s1 and 0 <= s1 < 2 ** 62
    for bad in (dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=-1.0), dict(do_sample=True, top_p=0.0),
                dict(do_sample=True, top_p=1.5)):
        with pytest.raises(ValueError):
            sel(**bad)
    assert sel(do_sample=False, num_beams=4) == ((False,), {})       # beam search: greedy token selection inside the steps, the beams live in generate()
    assert sel(do_sample=True, num_beams=4) == ((False,), {})        # beam-sample: the draw happens in beam.py on the steps' logits; the device sampler stays off


def test_beam_sample_warpers_and_draw():
    """Beam-sample (generate(num_beams = k, do_sample = True), transformers 4.40.1 _beam_sample restated in beam.py): (1) warp_scores keeps exactly the
    set the installed transformers' warpers keep (temperature -> top-k -> top-p, min_tokens_to_keep = 2) and gives the same values; (2) with top_k = 1 ...
    there is nothing to draw from but the k best, so the sampled search walks the same candidates as the deterministic one; (3) a seeded run is
    reproducible, different seeds explore different sequences, and every returned sequence is a valid hypothesis (length, eos rule)."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from grounded_video_llm_amd.beam import beam_search, warp_scores
    g = torch.Generator(); g.manual_seed(3)
    lp = torch.log_softmax(torch.randn((5, 97), generator=g) * 3.0, dim=-1)
    for T, tk, tp in ((1.0, 50, None), (0.2, 50, None), (0.7, None, 0.9), (1.3, 7, 0.5), (1.0, 1, 0.01)):
        ref = lp.clone()
        if T != 1.0:
            ref = TemperatureLogitsWarper(T)(None, ref)
        if tk:
            ref = TopKLogitsWarper(top_k=tk, min_tokens_to_keep=2)(None, ref)
        if tp is not None:
            ref = TopPLogitsWarper(top_p=tp, min_tokens_to_keep=2)(None, ref)
        got = warp_scores(lp, T, tk, tp)
        assert torch.equal(torch.isinf(got), torch.isinf(ref)), (T, tk, tp)
        assert torch.allclose(got[~torch.isinf(got)], ref[~torch.isinf(ref)], rtol=0, atol=1e-6)
    # a toy "model": next-token logits depend on the last token only
    V, k = 31, 3
    table = torch.randn((V, V), generator=g) * 2.0
    first = torch.randn((V,), generator=g) * 2.0

    def run(sample, eos=None, mx=6):
        seqs = [[] for _ in range(k)]

        def step(parents, toks):
            seqs[:] = [seqs[p_] + [t] for p_, t in zip(parents, toks)]
            return torch.stack([table[s_[-1]] for s_ in seqs])
        return beam_search(step, first, k, mx, eos, 1.0, False, sample)

    def smp(seed, **kw):
        gg = torch.Generator(); gg.manual_seed(seed)
        return dict(temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 50), top_p=kw.get("top_p"), generator=gg)
    a = run(smp(5))
    assert a == run(smp(5)) and len(a) == 6 and all(0 <= t < V for t in a)
    assert len({tuple(run(smp(sd, temperature=2.0))) for sd in range(8)}) > 1
    eos = run(None)[2]
    out = run(smp(1), eos=eos, mx=9)
    assert 1 <= len(out) <= 9 and (eos not in out[:-1])
    # temperature -> 0 sharpens every beam's distribution onto its best token: the draw degenerates to the k beams' argmax candidates
    cold = run(smp(9, temperature=1e-3, top_k=2))
    assert len(cold) == 6
    # 4.40.1's _beam_sample starts every beam at score 0: the first draw is over k identical rows, so every first-step parent is the prompt (0)
    # whichever row a pick came from -- the caller holds ONE sequence at that point (model.beam_generate_ids) -- and duplicates are legal
    first_parents = []

    def step_rec(parents, toks):
        if not first_parents:
            first_parents.extend(parents)
        return torch.stack([table[t] for t in toks])
    beam_search(step_rec, first, k, 3, None, 1.0, False, smp(2, temperature=3.0))
    assert first_parents == [0] * k
    # every row keeps min_tokens_to_keep = 2 candidates, so with all k rows live from the first step (scores 0) the 2k draws always exist -- the case
    # ADVICE r4 describes (top_p small at temperature 0.2, k >= 3: two finite candidates in the one live row) is gone with the -1e9 initialisation;
    # beam_search still refuses to draw from fewer than 2k finite entries instead of trusting torch.multinomial's silent zero-probability picks
    out = beam_search(step_rec, first, 4, 3, None, 1.0, False, smp(2, temperature=0.2, top_k=1, top_p=0.01))
    assert len(out) == 3


def test_beam_search_bookkeeping_equals_hf_generate():
    """grounded_video_llm_amd/beam.py restates transformers 4.40.1's BeamSearchScorer / BeamHypotheses (the version the reference pins; the installed 5.x
    has no such class any more).  Pin: the SAME tiny LlamaForCausalLM drives this function (logits by full re-forward per beam) and the installed
    transformers' own generate(inputs_embeds=..., num_beams=k, do_sample=False) -- the sequences must be equal for k = 2, 3, 4, with and without an eos
    id, length_penalty 1 and 2."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from grounded_video_llm_amd.beam import beam_search
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=256)
    m = LlamaForCausalLM(cfg).eval()
    E = m.get_input_embeddings().weight
    n_eos_hits = 0
    for seed in range(6):
        emb = torch.randn((1, 7, 32), generator=torch.Generator().manual_seed(seed)) * 2.0
        with torch.no_grad():                                            # an eos id the model really produces: the third token of the eos-free 3-beam answer
            free = m.generate(inputs_embeds=emb, num_beams=3, do_sample=False, max_new_tokens=8, eos_token_id=None, pad_token_id=0)[0].tolist()
        for k, eos, mx, lp in ((3, free[2], 9, 1.0), (4, None, 6, 1.0), (2, free[2], 12, 1.0), (3, free[1], 10, 2.0), (4, free[3], 10, 0.5)):
            with torch.no_grad():
                ref = m.generate(inputs_embeds=emb, num_beams=k, do_sample=False, max_new_tokens=mx, eos_token_id=eos, pad_token_id=0, length_penalty=lp, early_stopping=False)[0].tolist()

            def fwd(x):
                with torch.no_grad():
                    return m(inputs_embeds=x).logits[0, -1]
            beams = [[] for _ in range(k)]

            def step(parents, toks):
                beams[:] = [beams[p_] + [t] for p_, t in zip(parents, toks)]
                return torch.stack([fwd(torch.cat([emb, E[torch.tensor(b)][None]], 1)) for b in beams])
            got = beam_search(step, fwd(emb), k, mx, eos, lp, False)
            while ref and ref[-1] == 0 and len(ref) > len(got):          # HF pads the batch row to the longest hypothesis
                ref = ref[:-1]
            assert got == ref, (seed, k, eos, mx, lp, got, ref)
            n_eos_hits += int(eos is not None and eos in got)
    assert n_eos_hits >= 1, "no case ended by eos: the hypothesis bookkeeping was not exercised"


def test_step_only_trace_window(tmp_path):
    """tools/rocpd_stats.py --between ("trace the step alone"): only dispatches that start between the first and the last marker kernel
    are summarised, the markers themselves are left out, and the header counts foreign (at::native / rocclr) dispatches inside the window."""
    import sqlite3
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import rocpd_stats
    db = str(tmp_path / "t.db")
    con = sqlite3.connect(db)
    con.execute("create table kernels (name text, start integer, end integer)")
    rows = [("void at::native::fill<float>(...)", 0, 50_000), ("__amd_rocclr_fillBufferAligned", 60_000, 90_000),         # set-up: before the first marker
            ("gvl_trace_marker_kernel(int, int*)", 100_000, 101_000),
            ("void gemm_pp_kernel<256, 256, 64, 1>(GemmArgs, int, int)", 110_000, 1_110_000), ("attn_iv2_pipe_kernel<4>(AttnArgs)", 1_200_000, 1_700_000),
            ("void gemm_pp_kernel<256, 256, 64, 1>(GemmArgs, int, int)", 1_800_000, 2_800_000), ("__amd_rocclr_copyBuffer", 2_850_000, 2_860_000),
            ("gvl_trace_marker_kernel(int, int*)", 3_000_000, 3_001_000),
            ("void at::native::sum(...)", 3_100_000, 3_200_000)]                                                                  # extras: behind the last marker
    con.executemany("insert into kernels values (?, ?, ?)", rows)
    con.commit(); con.close()
    out = str(tmp_path / "o.txt")
    rocpd_stats.main(db, out, "gvl_trace_marker_kernel")
    txt = open(out).read()
    assert "over 4 dispatches" in txt and "total kernel time 2.510 ms" in txt
    assert "inside the window: 1" in txt                                  # the one blit kernel between the markers
    assert "at::native" not in txt.split("\n", 4)[4] and "gvl_trace_marker" not in txt.split("\n", 4)[4]
    gemm = [l for l in txt.splitlines() if l.startswith("void gemm_pp_kernel")][0].split()
    assert gemm[-6] == "2" and gemm[-5] == "2.000"                        # calls, total ms
    rocpd_stats.main(db, out)                                             # without the window: everything
    assert "over 9 dispatches" in open(out).read()
