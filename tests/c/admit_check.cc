// Drives the admission check (csrc/gvl_admit.h: host-only, no HIP) from a script on stdin: built with the host C++ compiler by tests/test_admit_cpu.py.
//   usage: admit_check <kv pages> <max sequences> <max_prefill> <max_seq> <outlist_cap> <vocab>
// One operation per line; every line is answered by one line "<rc>\t<message>": an id, 0 or a negative SeqStatus with an empty message -- or, for `admit`, the verdict.
//   open MAX | fork SRC N MAX | free SEQ | prefilled SEQ N (what a prefill of N rows leaves: pos N, n_gen 1, a bank's rows N) | bank SEQ (gvl_seq_keep_hidden)
//   pair LEAD FOLLOW | grammar SEQ (the sequence takes a new grammar) | set SEQ pos|ngen|rows|cap VALUE
//   fill_pages N | fill_slots N (sequences are opened until N pages / slots are free)
//   open_many SRC N MAX (SeqTable::open_many) | refusal FN STATUS (a SeqStatus as entry FN reports it)
//   admit ENTRY FN STRIDE N ID... [X...]   ENTRY: the index of gvl_admit::Entry; FN: the name a search passes, - for the entry's own; STRIDE 1: one number per member,
//     0: one number for all, -1: none
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>
#include "gvl_admit.h"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  SeqTable<> t(atoi(argv[2]), 4);
  t.reset_pool(atoi(argv[1]));
  const gvl_admit::Limits lim{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
  static char blob;
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string op; int a = 0, b = 0, c = 0;
    in >> op;
    int rc = -100;
    const char* msg = "";
    gvl_admit::Verdict v;
    if (op == "open") { in >> a; rc = t.open(a, -1, 0); }
    else if (op == "fork") { in >> a >> b >> c; rc = t.open(c, a, b); }
    else if (op == "free") { in >> a; rc = t.close(a); }
    else if (op == "prefilled") { in >> a >> b; SeqCore* s = t.lookup(a); if (!s) return 3; s->pos = b; s->n_gen = 1; if (s->bank_cap > 0) s->bank_rows = b; rc = 0; }
    else if (op == "bank") { in >> a; SeqCore* s = t.lookup(a); if (!s) return 3; s->bank_cap = s->max_tokens; s->bank_rows = 0; rc = 0; }
    else if (op == "pair") { in >> a >> b; if (!t.lookup(a) || !t.lookup(b)) return 3; t.lookup(a)->follow = b; t.lookup(b)->lead = a; rc = 0; }
    else if (op == "grammar") { in >> a; if (!t.lookup(a)) return 3; rc = t.set_grammar(t.lookup(a)->sel, t.add_grammar(&blob, lim.vocab)); }
    else if (op == "set") {
      std::string f; in >> a >> f >> b; SeqCore* s = t.lookup(a); if (!s) return 3;
      if (f == "pos") s->pos = b; else if (f == "ngen") s->n_gen = b; else if (f == "rows") s->bank_rows = b; else if (f == "cap") s->bank_cap = b; else return 4;
      rc = 0;
    }
    else if (op == "fill_pages") { in >> a; rc = 0; while ((int)t.free_pages.size() > a && rc >= 0) { const int n = (int)t.free_pages.size() - a; rc = t.open(64 * (n < 8 ? n : 8), -1, 0); } }
    else if (op == "fill_slots") {
      in >> a; rc = 0;
      for (;;) { int live = 0; for (const SeqCore& s : t.seqs) live += s.used; if (t.max_seqs - live <= a || rc < 0) break; rc = t.open(64, -1, 0); }
    }
    else if (op == "open_many") { in >> a >> b >> c; std::vector<int> ids(b > 0 ? b : 1); rc = t.open_many(a, b, c, ids.data()); }
    else if (op == "refusal") { std::string fn; in >> fn >> a; v = gvl_admit::seq_refusal(fn.c_str(), a); rc = v.status; msg = v.message; }
    else if (op == "admit") {
      std::string fn; int e = 0, stride = 0, n = 0;
      in >> e >> fn >> stride >> n;
      if (e < 0 || e >= gvl_admit::N_ENTRIES || n < 0) return 5;
      std::vector<int> ids(n), xs(stride == 1 ? n : (stride == 0 ? 1 : 0));
      for (int& x : ids) in >> x;
      for (int& x : xs) in >> x;
      if (!in) return 6;
      v = gvl_admit::admit(t, (gvl_admit::Entry)e, ids.data(), n, xs.empty() ? nullptr : xs.data(), stride == 1 ? 1 : 0, lim, fn == "-" ? nullptr : fn.c_str());
      rc = v.status; msg = v.message;
    }
    else return 4;
    printf("%d\t%s\n", rc, msg);
  }
  return 0;
}
