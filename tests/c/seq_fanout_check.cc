// Drives the fan-out operation of the sequence table (SeqTable::fanout, csrc/gvl_seq_table.h: host-only, no HIP) from a script on stdin: built with the host C++ compiler by
// tests/test_seq_fanout_cpu.py.
//   usage: seq_fanout_check <kv pages> <max sequences>
// One operation per line; every line is answered by one JSON object: the result code "rc" (0, an id, or a negative SeqStatus), "ids" (the siblings of a fanout) and the table.
//   alloc MAX | prefill SEQ N (the sequence now holds N tokens and its first generated id) | step SEQ (one more token and id) | free SEQ | pair LEAD FOLLOW
//   fanout SRC N MAX STREAM0 (sibling i draws from stream STREAM0 + i; N <= 64)
//   own SEQ ON TEMP TOPK SEED STREAM (a sampling setting of the sequence's own) | ctx ON TEMP TOPK SEED (the table-wide setting the others follow)
//   newrules | rules SEQ ID | newgrammar | grammar SEQ ID | topn SEQ N | proc SEQ PENALTY NGRAM MIN_NEW EOS
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include "gvl_seq_table.h"

static void dump_ints(const std::vector<int>& v) { printf("["); for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? "," : "", v[i]); printf("]"); }
static void dump_sel(const SeqSelect& s) {
  printf("{\"proc\":[%.9g,%d,%d,%d],\"top_n\":%d,\"rules\":%d,\"grammar\":%d,\"own\":%d,\"sampling\":[%d,%.9g,%d,%llu,%u]}", (double)s.proc.penalty, s.proc.ngram, s.proc.min_new,
         s.proc.eos, s.top_n, s.rules, s.grammar, (int)s.own_sampling, (int)s.sampling.on, (double)s.sampling.inv_temp, s.sampling.top_k, s.sampling.seed, s.sampling.stream);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  SeqTable<> t(atoi(argv[2]), 8, 8);
  t.reset_pool(atoi(argv[1]));
  static char blobs[64];
  int n_blobs = 0;
  Sampling ctx_setting;
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string op; int a = 0, b = 0, c = 0, d = 0;
    in >> op;
    int rc = -100;
    std::vector<int> ids;
    if (op == "alloc") { in >> a; rc = t.open(a, -1, 0); }
    else if (op == "prefill") { in >> a >> b; rc = t.lookup(a) ? (t.lookup(a)->pos = b, t.lookup(a)->n_gen = 1, 0) : (int)SEQ_BAD; }
    else if (op == "step") { in >> a; rc = t.lookup(a) ? (++t.lookup(a)->pos, ++t.lookup(a)->n_gen, 0) : (int)SEQ_BAD; }
    else if (op == "free") { in >> a; rc = t.close(a); }
    else if (op == "pair") { in >> a >> b; rc = t.lookup(a) && t.lookup(b) ? (t.lookup(a)->follow = b, t.lookup(b)->lead = a, 0) : (int)SEQ_BAD; }
    else if (op == "fanout") {
      in >> a >> b >> c >> d;
      if (b > 64) return 3;
      unsigned streams[64]; int out[64];
      for (int i = 0; i < 64; ++i) { streams[i] = (unsigned)(d + i); out[i] = -7; }
      rc = t.fanout(a, b, c, ctx_setting, streams, out);
      if (rc == SEQ_OK) ids.assign(out, out + b);
      else for (int i = 0; i < 64; ++i) if (out[i] != -7) return 6;          // a refusal writes no id
    }
    else if (op == "own" || op == "ctx") {
      Sampling q; double temp; unsigned long long seed; unsigned stream = 0; int on;
      if (op == "own") in >> a;
      in >> on >> temp >> b >> seed;
      if (op == "own") in >> stream;
      q.on = on != 0; q.inv_temp = (float)(1.0 / temp); q.top_k = b; q.seed = seed; q.stream = stream;
      if (op == "ctx") { ctx_setting = q; rc = 0; }
      else rc = t.lookup(a) ? (t.set_sampling(t.lookup(a)->sel, &q), 0) : (int)SEQ_BAD;
    }
    else if (op == "newrules") { rc = t.add_rules(&blobs[n_blobs]); if (rc >= 0) ++n_blobs; }
    else if (op == "rules") { in >> a >> b; rc = t.lookup(a) ? t.set_rules(t.lookup(a)->sel, b) : (int)SEQ_BAD; }
    else if (op == "newgrammar") { rc = t.add_grammar(&blobs[n_blobs], 32); if (rc >= 0) ++n_blobs; }
    else if (op == "grammar") { in >> a >> b; rc = t.lookup(a) ? t.set_grammar(t.lookup(a)->sel, b) : (int)SEQ_BAD; }
    else if (op == "topn") { in >> a >> b; rc = t.lookup(a) ? (t.lookup(a)->sel.top_n = b, 0) : (int)SEQ_BAD; }
    else if (op == "proc") { double p; int e; in >> a >> p >> b >> c >> e; rc = t.lookup(a) ? (t.lookup(a)->sel.proc = LogitsProc{(float)p, b, c, e}, 0) : (int)SEQ_BAD; }
    else return 4;
    printf("{\"rc\":%d,\"ids\":", rc); dump_ints(ids);
    printf(",\"free\":"); dump_ints(t.free_pages);
    printf(",\"ref\":"); dump_ints(t.page_ref);
    printf(",\"seqs\":{");
    bool first = true;
    for (size_t i = 0; i < t.seqs.size(); ++i) {
      const SeqCore& s = t.seqs[i];
      if (!s.used) { if (s.max_tokens || s.pos || s.n_gen || !s.pages.empty() || s.sel.own_sampling || s.lead != -1 || s.follow != -1) return 5; continue; }   // a closed slot is reset
      printf("%s\"%d\":{\"max\":%d,\"pos\":%d,\"n_gen\":%d,\"lead\":%d,\"follow\":%d,\"pages\":", first ? "" : ",", (int)i, s.max_tokens, s.pos, s.n_gen, s.lead, s.follow); dump_ints(s.pages);
      printf(",\"sel\":"); dump_sel(s.sel); printf("}");
      first = false;
    }
    printf("},\"rule_refs\":[");
    for (size_t i = 0; i < t.rule_sets.size(); ++i) printf("%s%d", i ? "," : "", t.rule_sets[i].used ? t.rule_sets[i].refs : -1);
    printf("],\"grammar_refs\":[");
    for (size_t i = 0; i < t.grammars.size(); ++i) printf("%s%d", i ? "," : "", t.grammars[i].used ? t.grammars[i].refs : -1);
    printf("]}\n");
  }
  return 0;
}
