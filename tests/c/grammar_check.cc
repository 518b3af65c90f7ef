// grammar_check.cc -- decoding grammars (csrc/gvl_grammar.h) and their reference counts (csrc/gvl_seq_table.h) on the CPU, no HIP.
//   grammar_check selftest   the checker's errors and limits, hand-written walks and allowed sets, the blob round trip, reference counts across open / fork / clone /
//                            close / destroy.  Prints one line per check; the exit status is the number of the first failed check (0: all passed).
//   grammar_check eval       reads one description and histories from stdin and prints what the header's check / walk / allowed say, one JSON line each -- the Python
//                            mirror (grounded_video_llm_amd/grammar.py) is compared with it.  Input: "n_states n_classes start vocab n_tc n_base n_trans", then n_tc
//                            classes, n_base bases, n_trans entries, then the number of histories and each as "len id id ...".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "gvl_grammar.h"
#include "gvl_seq_table.h"

namespace gg = gvl_grammar;
static int n_check = 0;
#define CHECK(cond) do { ++n_check; if (!(cond)) { printf("FAILED %d: %s\n", n_check, #cond); return n_check; } printf("ok %d: %s\n", n_check, #cond); } while (0)

struct G {
  int ns, nc, start, vocab;
  std::vector<uint8_t> tc; std::vector<int32_t> base; std::vector<uint16_t> tr;
  G(int ns_, int nc_, int vocab_) : ns(ns_), nc(nc_), start(0), vocab(vocab_), tc((size_t)vocab_, 0), base((size_t)nc_, -1), tr((size_t)ns_ * nc_, gg::FORBIDDEN) {}
  gg::Desc desc() const { return gg::Desc{ns, nc, start, vocab, tc.data(), base.data(), tr.data()}; }
  uint16_t& e(int s, int c) { return tr[(size_t)s * nc + c]; }
  std::string check() const { return gg::check(desc()); }
  bool has(const char* what) const { return check().find(what) != std::string::npos; }
};
using V = std::vector<int>;

// vocab 12: class 0 = ids 0, 1 (plain), class 1 = ids 2 .. 9 (ordinal, base 2), class 2 = id 10 (eos), class 3 = id 11 (plain, never allowed)
// state 0 --class 1, SET--> 1 --class 0--> 2 --class 1, GE--> 3 --class 2--> 4 (END)
static G interval() {
  G g(5, 4, 12);
  for (int t = 2; t < 10; ++t) g.tc[t] = 1;
  g.tc[10] = 2; g.tc[11] = 3; g.base[1] = 2;
  g.e(0, 1) = 1 | gg::SET; g.e(1, 0) = 2; g.e(2, 1) = 3 | gg::GE; g.e(3, 2) = 4;
  return g;
}
// the ids the mask keeps after history h; {-1}: nothing is masked (OFF or END)
static V allowed_ids(const gg::Desc& d, const std::vector<int32_t>& h) {
  const gg::Walk w = gg::walk(d, h.data(), (int)h.size());
  if (!gg::masks(d, w)) return V{-1};
  V out;
  for (int t = 0; t < d.vocab; ++t) if (gg::allowed(d, w, t)) out.push_back(t);
  return out;
}

static int selftest() {
  // ---- the checker: a valid grammar, then every error
  CHECK(interval().check() == "");
  { G g = interval(); g.ns = 0; CHECK(g.has("n_states is 0")); }
  { G g = interval(); g.nc = 0; CHECK(g.has("n_classes is 0")); }
  { G g = interval(); g.vocab = 0; CHECK(g.has("vocab is 0")); }
  { G g = interval(); g.vocab = gg::MAX_VOCAB + 1; CHECK(g.has("vocab is 8388609")); }
  { G g = interval(); g.start = 5; CHECK(g.has("start state 5")); }
  { G g = interval(); g.start = -1; CHECK(g.has("start state -1")); }
  { G g = interval(); gg::Desc d = g.desc(); d.trans = nullptr; CHECK(gg::check(d) == "null array"); }
  { G g = interval(); g.tc[7] = 4; CHECK(g.has("token 7 has class 4")); }
  { G g = interval(); g.base[1] = -2; CHECK(g.has("class 1: base -2 out of range")); }
  { G g = interval(); g.base[1] = 5; CHECK(g.has("class 1: base 5 out of range")); }            // 8 ids from 5 run past the vocabulary
  { G g = interval(); g.base[1] = 1; CHECK(g.has("ordinal class 1 is not the contiguous id range 1 .. 8")); }
  { G g = interval(); g.tc[5] = 0; CHECK(g.has("ordinal class 1 is not the contiguous id range")); }   // a hole in the range
  { G g = interval(); g.e(1, 0) = 2 | gg::SET; CHECK(g.has("edge (state 1, class 0): SET / GE on a class that is not ordinal")); }
  { G g = interval(); g.e(1, 0) = 2 | gg::GE; CHECK(g.has("SET / GE on a class that is not ordinal")); }
  { G g = interval(); g.e(1, 0) = 5; CHECK(g.has("edge (state 1, class 0): next state 5 out of range")); }
  { G g = interval(); g.e(1, 0) = 2 | 0x400; CHECK(g.has("reserved bits set")); }
  // liveness: a GE edge alone is enough only on a class at least as large as every class with a SET edge
  { G g(3, 3, 12);                                     // class 1: ids 0 .. 7 (SET), class 2: ids 8 .. 10 (GE only), class 0: id 11
    for (int t = 0; t < 8; ++t) g.tc[t] = 1;
    for (int t = 8; t < 11; ++t) g.tc[t] = 2;
    g.base[1] = 0; g.base[2] = 8; g.e(0, 1) = 1 | gg::SET; g.e(1, 2) = 2 | gg::GE;
    CHECK(g.has("state 1 can forbid every token"));    // reg may reach 7, class 2 has ordinals 0 .. 2
    g.e(1, 0) = 1; CHECK(g.check() == "");             // an edge without GE on a non-empty class
    g.tc[11] = 2; CHECK(g.has("state 1 can forbid every token")); }   // ... but class 0 is empty now
  // ---- the limits, and one past each
  { G g(256, 16, 4); for (int s = 0; s < 256; ++s) g.e(s, 0) = (uint16_t)((s + 1) % 256); CHECK(g.check() == ""); }
  { G g(257, 1, 4); CHECK(g.has("n_states is 257")); }
  { G g(64, 64, 64); for (int s = 0; s < 64; ++s) g.e(s, 0) = (uint16_t)s; for (int t = 0; t < 64; ++t) g.tc[t] = (uint8_t)t; CHECK(g.check() == ""); }
  { G g(1, 65, 4); CHECK(g.has("n_classes is 65")); }
  { G g(241, 17, 4); CHECK(g.has("n_states * n_classes is 4097, the limit is 4096")); }
  { G g(128, 32, 4); for (int s = 0; s < 128; ++s) g.e(s, 0) = 0; CHECK(g.check() == ""); }      // 4096 entries exactly
  // ---- walks and allowed sets
  const G g = interval();
  const gg::Desc d = g.desc();
  CHECK(allowed_ids(d, {}) == (V{2, 3, 4, 5, 6, 7, 8, 9}));                          // empty history: any timestamp
  CHECK(allowed_ids(d, {6}) == (V{0, 1}));                                            // just after SET (reg 4)
  CHECK(allowed_ids(d, {6, 1}) == (V{6, 7, 8, 9}));                                   // GE: ordinal >= 4
  CHECK(allowed_ids(d, {2, 0}) == (V{2, 3, 4, 5, 6, 7, 8, 9}));                       // reg 0: every timestamp
  CHECK(allowed_ids(d, {9, 0}) == (V{9}));                                            // reg at the top: one id left
  CHECK(allowed_ids(d, {6, 1, 6}) == (V{10}));                                        // s == e passes; then eos only
  CHECK(allowed_ids(d, {6, 1, 7, 10}) == (V{-1}));                                    // END: nothing is masked
  CHECK(allowed_ids(d, {6, 1, 7, 10, 3}) == (V{-1}));                                 // past END: OFF
  CHECK(allowed_ids(d, {6, 1, 5}) == (V{-1}));                                        // GE fails: OFF
  CHECK(allowed_ids(d, {11}) == (V{-1}) && allowed_ids(d, {0}) == (V{-1}));           // forbidden ids: OFF
  CHECK(allowed_ids(d, {12}) == (V{-1}) && allowed_ids(d, {-1}) == (V{-1}));          // ids outside [0, vocab): OFF
  CHECK(allowed_ids(d, {6, 1, 5, 6}) == (V{-1}));                                     // OFF is for good
  { const int32_t h[3] = {6, 1, 8}; const gg::Walk w = gg::walk(d, h, 3);
    CHECK(w.on && w.state == 3 && w.reg == 4 && gg::masks(d, w) && !gg::is_end(d.trans, d.n_classes, 3) && gg::is_end(d.trans, d.n_classes, 4)); }
  { G loop(1, 1, 4); loop.e(0, 0) = 0;                                                // every id, forever: only the history cap ends it
    const gg::Desc ld = loop.desc();
    const std::vector<int32_t> h((size_t)gg::HIST_CAP + 1, 1);
    CHECK(gg::walk(ld, h.data(), gg::HIST_CAP).on && !gg::walk(ld, h.data(), gg::HIST_CAP + 1).on); }
  { G both(2, 1, 8); both.base[0] = 0; both.e(0, 0) = 0 | gg::SET | gg::GE;           // SET and GE on one edge: a non-decreasing run
    const gg::Desc bd = both.desc();
    CHECK(both.check() == "" && allowed_ids(bd, {1, 3, 3}) == (V{3, 4, 5, 6, 7}) && allowed_ids(bd, {3, 2}) == (V{-1})); }
  // ---- the device blob holds the description
  { const std::vector<uint32_t> w = gg::pack(d);
    gg::Header h; memcpy(&h, w.data(), sizeof(h));
    const gg::Desc u = gg::unpack(w.data());
    CHECK((int)w.size() == h.words && h.off_base == 8 && h.off_trans == 12 && h.off_class == 22 && h.words == 25);
    CHECK(u.n_states == 5 && u.n_classes == 4 && u.start == 0 && u.vocab == 12 && !memcmp(u.token_class, d.token_class, 12) && !memcmp(u.class_base, d.class_base, 16) &&
          !memcmp(u.trans, d.trans, 40));
    CHECK(allowed_ids(u, {6, 1}) == (V{6, 7, 8, 9})); }
  // ---- reference counts: exactly the rule sets' life cycle
  SeqTable<> t(8, 2, 2);
  t.reset_pool(16);
  int blob_a = 0, blob_b = 0;
  const int ga = t.add_grammar(&blob_a, 12), gb = t.add_grammar(&blob_b, 12);
  CHECK(ga == 0 && gb == 1 && t.add_grammar(nullptr, 12) == SEQ_GRAMMAR_FULL && t.grammars[ga].vocab == 12);
  CHECK(t.check_grammar(-1) == SEQ_OK && t.check_grammar(ga) == SEQ_OK && t.check_grammar(2) == SEQ_NO_GRAMMAR && t.check_grammar(-2) == SEQ_NO_GRAMMAR);
  const int s0 = t.open(100, -1, 0);
  CHECK(s0 >= 0 && t.lookup(s0)->sel.grammar == -1);                                   // the default: none
  CHECK(t.set_grammar(t.sel_default, ga) == SEQ_OK && t.grammars[ga].refs == 1);
  const int s1 = t.open(100, -1, 0);
  CHECK(s1 >= 0 && t.lookup(s1)->sel.grammar == ga && t.grammars[ga].refs == 2);       // sequences allocated AFTER take the default
  CHECK(t.lookup(s0)->sel.grammar == -1);
  CHECK(t.set_grammar(t.lookup(s0)->sel, gb) == SEQ_OK && t.grammars[gb].refs == 1);
  CHECK(t.set_grammar(t.lookup(s0)->sel, gb) == SEQ_OK && t.grammars[gb].refs == 1);   // the grammar it holds already: the count stays
  CHECK(t.set_grammar(t.lookup(s0)->sel, 7) == SEQ_NO_GRAMMAR && t.lookup(s0)->sel.grammar == gb && t.grammars[gb].refs == 1);
  // where a sequence's generated ids sit, and which forks of a sequence with a grammar would share some of them.  A prefill of 62 rows leaves pos 62, n_gen 1 (id 0
  // picked, not fed); eight steps later pos 70, n_gen 9: ids 0 .. 7 sit at positions 62 .. 69
  { SeqCore q; q.sel.grammar = gb;
    q.pos = 62; q.n_gen = 1; CHECK(t.first_generated(q) == 62 && !t.fork_cuts_answer(q, 0) && !t.fork_cuts_answer(q, 62));
    q.pos = 70; q.n_gen = 9; CHECK(t.first_generated(q) == 62 && !t.fork_cuts_answer(q, 62) && t.fork_cuts_answer(q, 63) && t.fork_cuts_answer(q, 64));
    q.pos = 64; q.n_gen = 0; CHECK(t.first_generated(q) == 64 && !t.fork_cuts_answer(q, 64));            // nothing generated (a sequence that was only forked / cloned)
    q.pos = 70; q.n_gen = 9; q.sel.grammar = -1; CHECK(!t.fork_cuts_answer(q, 64)); }                    // no grammar: forks are what they were
  t.lookup(s0)->pos = 70;
  const int fork = t.open(200, s0, 64), clone = t.open(200, s0, 70);
  CHECK(fork >= 0 && clone >= 0 && t.lookup(fork)->sel.grammar == gb && t.lookup(clone)->sel.grammar == gb && t.grammars[gb].refs == 3);
  CHECK(t.destroy_grammar(gb, nullptr) == SEQ_GRAMMAR_BUSY && t.destroy_grammar(ga, nullptr) == SEQ_GRAMMAR_BUSY);
  CHECK(t.close(s0) == SEQ_OK && t.grammars[gb].refs == 2 && t.seqs[s0].sel.grammar == -1);   // a closed slot is reset
  CHECK(t.close(fork) == SEQ_OK && t.destroy_grammar(gb, nullptr) == SEQ_GRAMMAR_BUSY);        // the clone still holds it
  CHECK(t.set_grammar(t.lookup(clone)->sel, -1) == SEQ_OK && t.grammars[gb].refs == 0);
  void* blob = nullptr;
  CHECK(t.destroy_grammar(gb, nullptr) == SEQ_OK && t.grammars[gb].used);                      // asking does not destroy
  CHECK(t.destroy_grammar(gb, &blob) == SEQ_OK && blob == &blob_b && !t.grammars[gb].used && t.destroy_grammar(gb, &blob) == SEQ_NO_GRAMMAR);
  CHECK(t.set_grammar(t.lookup(clone)->sel, gb) == SEQ_NO_GRAMMAR);
  CHECK(t.close(s1) == SEQ_OK && t.grammars[ga].refs == 1 && t.destroy_grammar(ga, nullptr) == SEQ_GRAMMAR_BUSY);   // the default still holds it
  CHECK(t.set_grammar(t.sel_default, -1) == SEQ_OK && t.destroy_grammar(ga, &blob) == SEQ_OK && blob == &blob_a);
  CHECK(t.add_grammar(nullptr, 5) == 0);                                                       // a freed slot is taken again
  CHECK(t.lookup(clone)->sel.rules == -1 && t.rule_sets.empty() && t.close(clone) == SEQ_OK && !t.any_live() && t.free_pages.size() == 16);
  return 0;
}

static int eval() {
  int ns, nc, start, vocab, n_tc, n_base, n_tr, v;
  if (scanf("%d %d %d %d %d %d %d", &ns, &nc, &start, &vocab, &n_tc, &n_base, &n_tr) != 7) return 2;
  std::vector<uint8_t> tc; std::vector<int32_t> base; std::vector<uint16_t> tr;
  for (int i = 0; i < n_tc; ++i) { if (scanf("%d", &v) != 1) return 2; tc.push_back((uint8_t)v); }
  for (int i = 0; i < n_base; ++i) { if (scanf("%d", &v) != 1) return 2; base.push_back(v); }
  for (int i = 0; i < n_tr; ++i) { if (scanf("%d", &v) != 1) return 2; tr.push_back((uint16_t)v); }
  const gg::Desc d{ns, nc, start, vocab, tc.data(), base.data(), tr.data()};
  const std::string msg = gg::check(d);
  printf("{\"check\": \"%s\"}\n", msg.c_str());
  if (!msg.empty()) return 0;
  int nh;
  if (scanf("%d", &nh) != 1) return 2;
  for (int q = 0; q < nh; ++q) {
    int len;
    if (scanf("%d", &len) != 1) return 2;
    std::vector<int32_t> h;
    for (int i = 0; i < len; ++i) { if (scanf("%d", &v) != 1) return 2; h.push_back(v); }
    const gg::Walk w = gg::walk(d, h.data(), len);
    printf("{\"on\": %d, \"state\": %d, \"reg\": %d, \"allowed\": [", (int)w.on, w.state, w.reg);
    const V a = allowed_ids(d, h);
    for (size_t i = 0; i < a.size(); ++i) printf("%s%d", i ? ", " : "", a[i]);
    printf("]}\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc == 2 && !strcmp(argv[1], "eval")) return eval();
  fprintf(stderr, "usage: grammar_check selftest | eval\n");
  return 2;
}
