// Drives the operator entries' checks (csrc/gvl_op_check.h: host-only, no HIP) from a script on stdin: built with the host C++ compiler by tests/test_op_check_cpu.py.
// One case per line, answered by one line "<status>\t<message>": 0 and nothing, or -1 (GVL_ERR_ARG) and the entry's whole message -- what gvl_op_<entry> answers before
// it launches: check_<entry> on the descriptor, then, for the four entries that read pos and their block tables back, tables_<entry> on the host copies.
//   ENTRY FIELD=VALUE ... #ARRAY=V,V,...
//   ENTRY   patch_embed | decode_proj | decode_attention | qkv_post | prefill_attention | iv2_attention
//   FIELD   a field of the entry's descriptor (include/gvl.h); left out: zero / null.  An int: N=48; a pointer: W=@LOW -- set, LOW its low four address bits -- (the
//           driver makes up an address with those bits); an int array: vl_rows=0,3,68; a pointer array: vl_tables=@0,-,@0 (-: null).  Floats are not given: no check reads one
//   #ARRAY  what the entry would read back: #pos, #tables (decode_proj, decode_attention), #block_table, #vl0 .. #vl7 (qkv_post, prefill_attention).  Each is copied
//           into an allocation of exactly the size the entry reads (zero-filled where the script gives less), so a sanitizer sees a walk that leaves it
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "gvl_op_check.h"

namespace {

struct Field { const char* name; char kind; size_t off; };   // kind: i int32, p pointer, I int32 array, P pointer array
#define F(S, k, f) {#f, k, offsetof(S, f)}

const Field kPatch[] = {F(gvl_patch_embed, 'i', mode), F(gvl_patch_embed, 'i', path), F(gvl_patch_embed, 'i', n), F(gvl_patch_embed, 'i', T), F(gvl_patch_embed, 'i', image),
  F(gvl_patch_embed, 'i', patch), F(gvl_patch_embed, 'i', C), F(gvl_patch_embed, 'i', Kp), F(gvl_patch_embed, 'p', px), F(gvl_patch_embed, 'p', W), F(gvl_patch_embed, 'p', bias),
  F(gvl_patch_embed, 'p', cls), F(gvl_patch_embed, 'p', pos), F(gvl_patch_embed, 'p', lnw), F(gvl_patch_embed, 'p', lnb), F(gvl_patch_embed, 'p', out), F(gvl_patch_embed, 'p', im2col)};
#define DP(k, f) F(gvl_decode_proj, k, f)
const Field kProj[] = {DP('i', path), DP('i', variant), DP('i', w_fmt), DP('i', N), DP('i', K), DP('i', batch), DP('p', W), DP('p', x), DP('i', x_is_tiled), DP('i', act), DP('p', bias),
  DP('p', resid), DP('p', out_bf16), DP('p', out_f32), DP('i', out_tiled), DP('i', out_stride), DP('p', norm_w), DP('i', sq_n), DP('p', sq_in), DP('p', sq_out), DP('p', out_tiled2),
  DP('i', rope_on), DP('i', rope_switch), DP('p', cos_s), DP('p', sin_s), DP('p', cos_l), DP('p', sin_l), DP('i', max_pos), DP('i', n_pages), DP('p', pos), DP('p', tables),
  DP('i', table_stride), DP('i', q_stride), DP('p', Q), DP('p', Kt), DP('p', Vt), DP('i', H), DP('i', KV), DP('i', Dr), DP('i', D), DP('p', w_deq), DP('p', w_scale)};
#define DA(k, f) F(gvl_decode_attn, k, f)
const Field kDecAttn[] = {DA('p', q), DA('p', Kt), DA('p', Vt), DA('p', tables), DA('p', pos), DA('p', part), DA('p', counters), DA('p', out), DA('i', q_stride), DA('i', n_pages),
  DA('i', table_stride), DA('i', out_stride), DA('i', out_tiled), DA('i', batch), DA('i', H), DA('i', KV), DA('i', D), DA('i', Dout), DA('i', nsplit), DA('i', hpb), DA('i', cpb), DA('i', gsplit)};
#define QP(k, f) F(gvl_qkv_post, k, f)
const Field kQkv[] = {QP('p', qkv), QP('i', ld), QP('p', Q), QP('p', Kt), QP('p', Vt), QP('p', block_table), QP('i', max_pages), QP('i', B), QP('i', S), QP('i', H), QP('i', KV), QP('i', Dr),
  QP('i', D), QP('i', mode), QP('p', qn), QP('p', kn), QP('p', cos), QP('p', sin), QP('i', pos0), QP('i', ones_row), QP('i', k_ones), QP('p', q_rs), QP('i', vl_n), QP('I', vl_rows),
  QP('P', vl_tables), QP('I', vl_pos0), QP('I', table_len), QP('i', n_pages), QP('i', max_pos), QP('i', ext)};
#define PA(k, f) F(gvl_prefill_attn, k, f)
const Field kPrefill[] = {PA('p', Q), PA('p', Kt), PA('p', Vt), PA('p', O), PA('p', block_table), PA('i', max_pages), PA('i', B), PA('i', H), PA('i', KV), PA('i', S), PA('i', D), PA('i', Dout),
  PA('i', Sk), PA('i', qpos0), PA('i', causal), PA('i', ring), PA('i', vl_n), PA('I', vl_rows), PA('P', vl_tables), PA('I', vl_pos0), PA('I', table_len), PA('i', ext), PA('i', n_pages)};
#define IV(k, f) F(gvl_iv2_attn, k, f)
const Field kIv2[] = {IV('p', qkv), IV('i', ld), IV('p', Q), IV('p', Kt), IV('p', Vt), IV('p', q_rs), IV('p', q_nw), IV('p', out), IV('i', B), IV('i', S), IV('i', H), IV('i', Dr), IV('i', form),
  IV('i', pipe), IV('i', pipe_rows)};

alignas(16) char g_somewhere[64];
const void* address(const std::string& v) { return v == "-" ? nullptr : g_somewhere + 16 + (atoi(v.c_str() + 1) & 15); }   // "@LOW"

std::vector<std::string> split(const std::string& s) {
  std::vector<std::string> out; std::string x; std::istringstream in(s);
  while (std::getline(in, x, ',')) out.push_back(x);
  return out;
}
template <size_t N>
bool fill(void* desc, const Field (&fields)[N], const std::string& key, const std::string& val) {
  for (const Field& f : fields) {
    if (key != f.name) continue;
    char* at = (char*)desc + f.off;
    const std::vector<std::string> vs = split(val);
    if (f.kind == 'i') { const int32_t x = (int32_t)atoll(val.c_str()); memcpy(at, &x, 4); }
    else if (f.kind == 'p') { const void* p = address(val); memcpy(at, &p, sizeof p); }
    else if (f.kind == 'I') { if (vs.size() > (key == "vl_rows" ? 9u : 8u)) return false; for (size_t i = 0; i < vs.size(); ++i) { const int32_t x = (int32_t)atoll(vs[i].c_str()); memcpy(at + 4 * i, &x, 4); } }
    else { if (vs.size() > 8) return false; for (size_t i = 0; i < vs.size(); ++i) { const void* p = address(vs[i]); memcpy(at + sizeof p * i, &p, sizeof p); } }
    return true;
  }
  return false;
}
using Arrays = std::map<std::string, std::vector<int>>;
// the script's array `name` in an allocation of exactly `count` ints
std::vector<int> exactly(const Arrays& a, const std::string& name, long long count) {
  std::vector<int> v((size_t)(count > 0 ? count : 0), 0);
  auto it = a.find(name);
  if (it != a.end()) for (size_t i = 0; i < v.size() && i < it->second.size(); ++i) v[i] = it->second[i];
  return v;
}
template <class P>
const char* paged(const P& p, const Arrays& a, const char* (*tables)(const P&, const gvl_op::HostTables&)) {
  gvl_op::HostTables h{};
  const std::vector<int> block = exactly(a, "block_table", !p.vl_n && p.block_table ? (long long)p.B * p.max_pages : 0);
  std::vector<int> vl[GVL_MAX_PREFILL_BATCH];
  h.block = block.empty() ? nullptr : block.data();
  for (int u = 0; u < p.vl_n && p.table_len[u] >= 1; ++u) { vl[u] = exactly(a, "vl" + std::to_string(u), p.table_len[u]); h.vl[u] = vl[u].data(); }
  return tables(p, h);
}

}  // namespace

int main() {
  std::string line;
  char buf[1 << 16];
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string entry, tok;
    in >> entry;
    gvl_patch_embed pe; gvl_decode_proj dp; gvl_decode_attn da; gvl_qkv_post qp; gvl_prefill_attn pa; gvl_iv2_attn iv;
    memset(&pe, 0, sizeof pe); memset(&dp, 0, sizeof dp); memset(&da, 0, sizeof da); memset(&qp, 0, sizeof qp); memset(&pa, 0, sizeof pa); memset(&iv, 0, sizeof iv);
    Arrays arrays;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) return 3;
      const std::string key = tok.substr(0, eq), val = tok.substr(eq + 1);
      if (key[0] == '#') { std::vector<int>& v = arrays[key.substr(1)]; for (const std::string& x : split(val)) v.push_back((int)atoll(x.c_str())); continue; }
      const bool ok = entry == "patch_embed" ? fill(&pe, kPatch, key, val) : entry == "decode_proj" ? fill(&dp, kProj, key, val) : entry == "decode_attention" ? fill(&da, kDecAttn, key, val)
                    : entry == "qkv_post" ? fill(&qp, kQkv, key, val) : entry == "prefill_attention" ? fill(&pa, kPrefill, key, val) : entry == "iv2_attention" ? fill(&iv, kIv2, key, val) : false;
      if (!ok) { fprintf(stderr, "op_check: %s has no field %s (or too many values)\n", entry.c_str(), key.c_str()); return 4; }
    }
    const char* bad = nullptr;
    if (entry == "patch_embed") bad = gvl_op::check_patch_embed(pe);
    else if (entry == "iv2_attention") bad = gvl_op::check_iv2_attention(iv);
    else if (entry == "decode_proj") {
      bad = gvl_op::check_decode_proj(dp);
      if (!bad && dp.rope_on) {
        const std::vector<int> pos = exactly(arrays, "pos", dp.batch), tab = exactly(arrays, "tables", (long long)dp.batch * dp.table_stride);
        bad = gvl_op::tables_decode_proj(dp, pos.data(), tab.data());
      }
    } else if (entry == "decode_attention") {
      bad = gvl_op::check_decode_attention(da);
      if (!bad) {
        const std::vector<int> pos = exactly(arrays, "pos", da.batch), tab = exactly(arrays, "tables", (long long)da.batch * da.table_stride);
        bad = gvl_op::tables_decode_attention(da, pos.data(), tab.data());
      }
    } else if (entry == "qkv_post") {
      bad = gvl_op::check_qkv_post(qp);
      if (!bad) bad = paged(qp, arrays, gvl_op::tables_qkv_post);
    } else if (entry == "prefill_attention") {
      bad = gvl_op::check_prefill_attention(pa);
      if (!bad) bad = paged(pa, arrays, gvl_op::tables_prefill_attention);
    } else return 5;
    if (bad) printf("-1\tgvl_op_%s: %s\n", entry.c_str(), bad);
    else printf("0\t\n");
  }
  return 0;
}
