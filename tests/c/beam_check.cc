// Drives csrc/gvl_beam.h (the host bookkeeping of gvl_beam_search) on a CPU: tests/test_beam_host_cpu.py replays the candidate lists beam.py saw and compares every line.
// stdin:  "k vocab max_new eos length_penalty early"            (eos -1 = none; early 0 False / 1 True / 2 "never"; floating-point fields in any strtod form, hex included)
//         then per step one line "n  v idx lp  v idx lp ..."    (n triples: candidate value, flat index, processed log-probability)
// stdout: per step "step rc done | parents | tokens"; after the step that finishes, "final score | ids | transition scores"; an error ends the run with "error rc text".
#include "gvl_beam.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  std::istringstream cfg(line);
  int k, vocab, max_new, eos, early; std::string lp;
  if (!(cfg >> k >> vocab >> max_new >> eos >> lp >> early)) return 2;
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
    std::printf("step %d %d |", rc, bs.done ? 1 : 0);
    for (int j = 0; j < k; ++j) std::printf(" %d", parents[j]);
    std::printf(" |");
    for (int j = 0; j < k; ++j) std::printf(" %d", tokens[j]);
    std::printf("\n");
    if (rc == gvl_beam::BEAM_FINISHED) {
      std::vector<int> ids; double score = 0.0; std::vector<float> ts;
      bs.finalize(&ids, &score, &ts);
      std::printf("final %.17g |", score);
      for (int t : ids) std::printf(" %d", t);
      std::printf(" |");
      for (float t : ts) std::printf(" %.17g", (double)t);
      std::printf("\n");
      return 0;
    }
  }
  return 0;
}
