// Drives the sequence table (csrc/gvl_seq_table.h: host-only, no HIP) from a script on stdin: built with the host C++ compiler by tests/test_seq_table_cpu.py.
//   usage: seq_table_check <kv pages> <max sequences> <max rule sets>
// One operation per line; every line is answered by one JSON object: the result code "rc" (an id, 0, or a negative SeqStatus) and the whole table.
//   alloc MAX | fork SRC N MAX | clone SRC MAX | openmany SRC N MAX (N clones at once, all or nothing: 0 or a negative status) | free SEQ | pos SEQ N (the sequence now holds N tokens: what a prefill / decode leaves)
//   newrules | delrules ID | rules SEQ ID | topn SEQ N | proc SEQ PENALTY NGRAM MIN_NEW EOS      (SEQ -1: the default of later allocs)
//   pages SEQ CAP I | pagesnull SEQ CAP I: pages_of into 64 words filled with -77 (CAP -2: a null buffer with cap 0; pagesnull: a null count) -> a negative status, else
//     word I of the buffer afterwards (I -1: the count, -99 when it was not asked for)
//   live SEQ (0 / SEQ_BAD) | group SEQ... (the first member that is not live or repeats an earlier one decides: SEQ_BAD / SEQ_DUPLICATE)
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include "gvl_seq_table.h"

static void dump_sel(const SeqSelect& s) { printf("[%.9g,%d,%d,%d,%d,%d]", (double)s.proc.penalty, s.proc.ngram, s.proc.min_new, s.proc.eos, s.top_n, s.rules); }
static void dump_ints(const std::vector<int>& v) { printf("["); for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? "," : "", v[i]); printf("]"); }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  SeqTable<> t(atoi(argv[2]), atoi(argv[3]));
  t.reset_pool(atoi(argv[1]));
  static char blobs[1 << 16];            // rule-set blobs are opaque to the table: distinct addresses stand in for device memory
  int n_blobs = 0;
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string op; int a = 0, b = 0, c = 0;
    in >> op;
    int rc = -100;
    auto sel_of = [&](int seq) -> SeqSelect* { return seq == -1 ? &t.sel_default : (t.lookup(seq) ? &t.lookup(seq)->sel : nullptr); };
    if (op == "alloc") { in >> a; rc = t.open(a, -1, 0); }
    else if (op == "fork") { in >> a >> b >> c; rc = t.open(c, a, b); }
    else if (op == "clone") { in >> a >> b; rc = t.open(b, a, t.lookup(a) ? t.lookup(a)->pos : 0); }
    else if (op == "openmany") { in >> a >> b >> c; std::vector<int> ids(b > 0 ? b : 1, -1); rc = t.open_many(a, b, c, ids.data()); }
    else if (op == "free") { in >> a; rc = t.close(a); }
    else if (op == "pos") { in >> a >> b; rc = t.lookup(a) ? (t.lookup(a)->pos = b, 0) : (int)SEQ_BAD; }
    else if (op == "newrules") { rc = t.add_rules(&blobs[n_blobs]); if (rc >= 0) ++n_blobs; }
    else if (op == "delrules") {
      in >> a;
      const void* was = t.check_rules(a) == SEQ_OK && a >= 0 ? t.rule_sets[a].d : nullptr;
      void* d = nullptr;
      rc = t.destroy_rules(a, &d);
      if ((rc == SEQ_OK) != (d != nullptr) || (d && d != was)) return 3;      // the blob is handed back exactly when the set goes
    }
    else if (op == "rules") { in >> a >> b; SeqSelect* s = sel_of(a); rc = s ? t.set_rules(*s, b) : (int)SEQ_BAD; }
    else if (op == "topn") { in >> a >> b; SeqSelect* s = sel_of(a); rc = s ? (s->top_n = b, 0) : (int)SEQ_BAD; }
    else if (op == "proc") { double p; in >> a >> p >> b >> c; int e; in >> e; SeqSelect* s = sel_of(a); rc = s ? (s->proc = LogitsProc{(float)p, b, c, e}, 0) : (int)SEQ_BAD; }
    else if (op == "pages" || op == "pagesnull") {
      in >> a >> b >> c;
      int buf[64], n = -99;
      for (int& w : buf) w = -77;
      if (b > 64 || c < -1 || c >= 64) return 6;
      const int st = t.pages_of(a, b == -2 ? nullptr : buf, b == -2 ? 0 : b, op == "pages" ? &n : nullptr);
      rc = st < 0 ? st : (c == -1 ? n : buf[c]);
    }
    else if (op == "live") { in >> a; rc = t.lookup(a) ? SEQ_OK : SEQ_BAD; }
    else if (op == "group") {
      std::vector<int> ids; while (in >> a) ids.push_back(a);
      rc = SEQ_OK;
      for (int i = 0; i < (int)ids.size() && rc == SEQ_OK; ++i) rc = !t.lookup(ids[i]) ? SEQ_BAD : (t.repeats(ids.data(), i) ? SEQ_DUPLICATE : SEQ_OK);
    }
    else return 4;
    printf("{\"rc\":%d,\"any_live\":%d,\"slots\":%d,\"free\":", rc, (int)t.any_live(), (int)t.seqs.size()); dump_ints(t.free_pages);
    printf(",\"ref\":"); dump_ints(t.page_ref);
    printf(",\"default\":"); dump_sel(t.sel_default);
    printf(",\"seqs\":{");
    bool first = true;
    for (size_t i = 0; i < t.seqs.size(); ++i) {
      const SeqCore& s = t.seqs[i];
      if (!s.used) { if (s.max_tokens || s.n_pages || s.pos || s.n_gen || !s.pages.empty() || s.sel.rules != -1 || s.sel.top_n != -1 || s.sel.proc.on()) return 5; continue; }   // a closed slot is reset
      printf("%s\"%d\":{\"max\":%d,\"n_pages\":%d,\"pos\":%d,\"n_gen\":%d,\"pages\":", first ? "" : ",", (int)i, s.max_tokens, s.n_pages, s.pos, s.n_gen); dump_ints(s.pages);
      printf(",\"sel\":"); dump_sel(s.sel); printf("}");
      first = false;
    }
    printf("},\"rules\":{");
    first = true;
    for (size_t i = 0; i < t.rule_sets.size(); ++i) {
      if (!t.rule_sets[i].used) continue;
      printf("%s\"%d\":%d", first ? "" : ",", (int)i, t.rule_sets[i].refs);
      first = false;
    }
    printf("}}\n");
  }
  return 0;
}
