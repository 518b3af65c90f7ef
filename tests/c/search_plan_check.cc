// Drives the two pure pieces of csrc/gvl_beam.h the searches inside the library share, on a CPU, for tests/test_search_plan_cpu.py: the cache reorder's plan
// (gvl_beam::reorder) and the beam entries' value refusals (gvl_beam::refusal).
// stdin, one request per line:
//   "R k nb  b0 .. b(nb-1)  p0 .. p(k-1)"   beams (a sequence id, -1 closed) and parents (-1: the slot dies)
//        -> "ok | src .. | clones .. | closed .." or "error"
//   "V grouped k G lambda num_return vocab max_new max_new_cap cap early length_penalty penalty ngram min_new"   (floating-point fields in any strtod form)
//        -> the refusal's text, an empty line for none
#include "gvl_beam.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "R") {
      int k, nb;
      if (!(in >> k >> nb) || k < 0 || nb < 0) return 2;
      std::vector<int> beams(nb), parents(k);
      for (int& b : beams) if (!(in >> b)) return 2;
      for (int& p : parents) if (!(in >> p)) return 2;
      gvl_beam::ReorderPlan plan;
      if (!gvl_beam::reorder(beams, parents.data(), k, &plan)) { std::printf("error\n"); continue; }
      std::printf("ok |");
      for (int x : plan.src) std::printf(" %d", x);
      std::printf(" |");
      for (int x : plan.clones) std::printf(" %d", x);
      std::printf(" |");
      for (int x : plan.closed) std::printf(" %d", x);
      std::printf("\n");
    } else if (what == "V") {
      int grouped, k, G, nr, vocab, max_new, max_new_cap, cap, early, ngram, min_new; std::string lambda, lp, penalty;
      if (!(in >> grouped >> k >> G >> lambda >> nr >> vocab >> max_new >> max_new_cap >> cap >> early >> lp >> penalty >> ngram >> min_new)) return 2;
      const std::string why = gvl_beam::refusal(grouped != 0, k, G, (float)std::strtod(lambda.c_str(), nullptr), nr, vocab, max_new, max_new_cap, cap, early,
                                                std::strtod(lp.c_str(), nullptr), (float)std::strtod(penalty.c_str(), nullptr), ngram, min_new);
      std::printf("%s\n", why.c_str());
    } else {
      return 2;
    }
  }
  return 0;
}
