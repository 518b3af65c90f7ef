// Drives BeamState::finalize_n (csrc/gvl_beam.h, the n-best end of gvl_beam_search_n) on a CPU: tests/test_beam_nbest_cpu.py replays the candidate lists beam.py saw.
// stdin:  "k vocab max_new eos length_penalty early n"          (as tests/c/beam_check.cc, plus the number of hypotheses to return)
//         then per step one line "n  v idx lp  v idx lp ..."    (n triples: candidate value, flat index, processed log-probability)
// stdout: after the step that finishes, "count m", then m lines "final score | ids | transition scores" best first, then "best score | ids | transition scores" from
//         finalize() on a copy of the state; an error ends the run with "error rc text".
#include "gvl_beam.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

static void show(const char* tag, double score, const std::vector<int>& ids, const std::vector<float>& ts) {
  std::printf("%s %.17g |", tag, score);
  for (int t : ids) std::printf(" %d", t);
  std::printf(" |");
  for (float t : ts) std::printf(" %.17g", (double)t);
  std::printf("\n");
}

int main() {
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  std::istringstream cfg(line);
  int k, vocab, max_new, eos, early, n_ret; std::string lp;
  if (!(cfg >> k >> vocab >> max_new >> eos >> lp >> early >> n_ret)) return 2;
  gvl_beam::BeamState bs;
  const int rc0 = bs.init(k, vocab, max_new, eos, std::strtod(lp.c_str(), nullptr), early);
  if (rc0 < 0) { std::printf("error %d %s\n", rc0, gvl_beam::status_text(rc0)); return 0; }
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int n;
    if (!(in >> n)) continue;
    std::vector<float> vals(n), proc(n); std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) {
      std::string v, p;
      if (!(in >> v >> idx[i] >> p)) return 2;
      vals[i] = (float)std::strtod(v.c_str(), nullptr); proc[i] = (float)std::strtod(p.c_str(), nullptr);
    }
    std::vector<int> parents(k, -1), tokens(k, -1);
    const int rc = bs.step(vals.data(), idx.data(), proc.data(), n, parents.data(), tokens.data());
    if (rc < 0) { std::printf("error %d %s\n", rc, gvl_beam::status_text(rc)); return 0; }
    if (rc == gvl_beam::BEAM_FINISHED) {
      gvl_beam::BeamState one = bs;                       // finalize adds the open beams to the hypotheses: each end gets its own copy
      std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
      const int m = bs.finalize_n(n_ret, &ids, &score, &ts);
      std::printf("count %d\n", m);
      for (int r = 0; r < m; ++r) show("final", score[r], ids[r], ts[r]);
      std::vector<int> i1; double s1 = 0.0; std::vector<float> t1;
      one.finalize(&i1, &s1, &t1);
      show("best", s1, i1, t1);
      return 0;
    }
  }
  return 0;
}
