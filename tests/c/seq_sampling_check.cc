// seq_sampling_check.cc -- the sampling part of a sequence's settings (SeqSelect::own_sampling / sampling, csrc/gvl_seq_table.h) on the CPU: a new sequence follows the
// table-wide setting, gvl_seq_set_sampling's SeqTable::set_sampling gives it its own, fork and clone (SeqTable::open with a source) copy an own setting, a null setting restores
// following, and a closed slot is reset.  Prints one line per check; the exit status is the number of the first failed check (0: all passed).
#include <cstdio>
#include "gvl_seq_table.h"

static int n_check = 0;
#define CHECK(cond) do { ++n_check; if (!(cond)) { printf("FAILED %d: %s\n", n_check, #cond); return n_check; } printf("ok %d: %s\n", n_check, #cond); } while (0)

static bool same(const Sampling& a, const Sampling& b) {
  return a.on == b.on && a.inv_temp == b.inv_temp && a.top_k == b.top_k && a.top_p == b.top_p && a.min_p == b.min_p && a.typical_p == b.typical_p && a.eps == b.eps &&
         a.eta == b.eta && a.seed == b.seed && a.stream == b.stream;
}

int main() {
  SeqTable<> t(8, 2);
  t.reset_pool(16);
  const Sampling off;
  CHECK(!off.on && !off.warps());
  const int a = t.open(100, -1, 0);
  CHECK(a >= 0);
  CHECK(!t.lookup(a)->sel.own_sampling && same(t.lookup(a)->sel.sampling, off));            // a new sequence follows the default
  CHECK(!t.sel_default.own_sampling);
  Sampling q; q.on = true; q.inv_temp = 2.0f; q.top_k = 7; q.top_p = 0.9f; q.min_p = 0.05f; q.typical_p = 0.8f; q.eps = 1e-3f; q.eta = 2e-3f; q.seed = 0x123456789abcdefULL; q.stream = 3;
  CHECK(q.warps());
  Sampling plain = q; plain.min_p = plain.typical_p = plain.eps = plain.eta = 0.f;
  CHECK(plain.on && !plain.warps());
  Sampling one = plain; one.typical_p = 1.0f;
  CHECK(!one.warps());                                                                          // typical_p 1 is off
  t.set_sampling(t.lookup(a)->sel, &q);
  CHECK(t.lookup(a)->sel.own_sampling && same(t.lookup(a)->sel.sampling, q));
  const int fork = t.open(200, a, 64);                                                          // gvl_seq_fork: shares the first page
  CHECK(fork >= 0 && t.lookup(fork)->sel.own_sampling && same(t.lookup(fork)->sel.sampling, q));
  const int clone = t.open(100, a, 0);                                                          // gvl_seq_clone's table side: a source, nothing shared
  CHECK(clone >= 0 && t.lookup(clone)->sel.own_sampling && same(t.lookup(clone)->sel.sampling, q));
  Sampling q2 = q; q2.stream = 4;
  t.set_sampling(t.lookup(clone)->sel, &q2);                                                    // a different stream for the clone leaves the source alone
  CHECK(t.lookup(clone)->sel.sampling.stream == 4 && t.lookup(a)->sel.sampling.stream == 3 && t.lookup(fork)->sel.sampling.stream == 3);
  const int fresh = t.open(64, -1, 0);
  CHECK(fresh >= 0 && !t.lookup(fresh)->sel.own_sampling);                                      // own settings never leak into the default
  Sampling greedy;                                                                              // an own GREEDY setting is still an own setting
  t.set_sampling(t.lookup(fresh)->sel, &greedy);
  CHECK(t.lookup(fresh)->sel.own_sampling && !t.lookup(fresh)->sel.sampling.on);
  t.set_sampling(t.lookup(a)->sel, nullptr);
  CHECK(!t.lookup(a)->sel.own_sampling && same(t.lookup(a)->sel.sampling, off));            // null: back to following
  CHECK(t.lookup(fork)->sel.own_sampling);                                                      // the copies keep theirs
  const int after = t.open(100, a, 0);
  CHECK(after >= 0 && !t.lookup(after)->sel.own_sampling);                                      // a clone of a follower follows
  CHECK(t.close(fork) == SEQ_OK && !t.seqs[fork].used && !t.seqs[fork].sel.own_sampling && same(t.seqs[fork].sel.sampling, off));   // a closed slot is reset
  const int reuse = t.open(64, -1, 0);
  CHECK(reuse == fork && !t.lookup(reuse)->sel.own_sampling);
  CHECK(t.lookup(a)->sel.top_n == -1 && t.lookup(a)->sel.rules == -1 && !t.lookup(a)->sel.proc.on());   // the other settings are untouched
  printf("passed %d\n", n_check);
  return 0;
}
