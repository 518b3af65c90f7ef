// gvl_grammar.h -- decoding grammars (gvl_grammar_create, include/gvl.h): a DFA over token classes with one integer register, as the processor
// launch applies it (gvl_logits.hip).  Host-only, no HIP (tests/c/grammar_check.cc drives it on a CPU): the checker of a description, the packer of
// the device blob, and the reference walk() / allowed().  The kernel steps through the SAME pack_id / step / edge_allows / is_end below.
//
// Walk: start from (state = start, reg = 0) and feed the generated ids in order.  The walk turns OFF for good on an id outside [0, vocab), a forbidden
// transition, a GE transition with ordinal < reg, or a history longer than HIST_CAP.  A state whose whole row is forbidden is an END state.
// Mask: in an OFF or END state nothing is masked.  Otherwise id t is allowed iff its class's edge from the state is not forbidden and, on a GE
// edge, ordinal(t) >= reg.  On an edge with both flags the GE test reads the register before SET overwrites it.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define GVL_GRAMMAR_FN __host__ __device__ inline
#else
#define GVL_GRAMMAR_FN inline
#endif

namespace gvl_grammar {

constexpr int MAX_STATES = 256, MAX_CLASSES = 64, MAX_TRANS = 4096;   // MAX_TRANS uint16 entries = the kernel's 8 KB LDS table
constexpr int MAX_VOCAB = 1 << 23;                                    // class | ordinal << 8 stays a non-negative int32
constexpr int HIST_CAP = 8192;                                        // = GVL_LOGITS_HIST_CAP (gvl_internal.h asserts it)
constexpr uint16_t FORBIDDEN = 0xFFFF, NEXT_MASK = 0xFF, SET = 0x100, GE = 0x200;
constexpr int NO_CLASS = 0xFF;                                        // the packed entry of an id outside [0, vocab)

// gvl_grammar_desc's fields (include/gvl.h)
struct Desc {
  int32_t n_states, n_classes, start, vocab;
  const uint8_t* token_class;   // [vocab]
  const int32_t* class_base;    // [n_classes]: -1 plain; >= 0 ordinal, the ids base .. base + size - 1
  const uint16_t* trans;        // [n_states][n_classes]
};
// the device blob starts with this header; every off_* is a 32-bit word offset from the blob's start.  class_base [n_classes] int32, trans
// [n_states * n_classes] uint16, token_class [vocab] uint8, each padded to whole words
struct Header { int32_t n_states, n_classes, start, vocab, off_base, off_trans, off_class, words; };

GVL_GRAMMAR_FN bool edge_allows(uint16_t e, int ordinal, int reg) { return e != FORBIDDEN && (!(e & GE) || ordinal >= reg); }
// an id as the walk reads it: class | ordinal << 8 (ordinal 0 for a plain class); NO_CLASS outside [0, vocab)
GVL_GRAMMAR_FN int pack_id(int t, int vocab, const uint8_t* token_class, const int32_t* class_base) {
  if (t < 0 || t >= vocab) return NO_CLASS;
  const int c = token_class[t], b = class_base[c];
  return c | ((b >= 0 ? t - b : 0) << 8);
}
// one step of the walk on a packed id; false: the walk is OFF from here on
GVL_GRAMMAR_FN bool step(const uint16_t* trans, int n_classes, int& state, int& reg, int packed) {
  const int c = packed & 0xFF, ordinal = packed >> 8;
  if (c >= n_classes) return false;
  const uint16_t e = trans[state * n_classes + c];
  if (!edge_allows(e, ordinal, reg)) return false;
  if (e & SET) reg = ordinal;
  state = e & NEXT_MASK;
  return true;
}
GVL_GRAMMAR_FN bool is_end(const uint16_t* trans, int n_classes, int state) {
  for (int c = 0; c < n_classes; ++c) if (trans[state * n_classes + c] != FORBIDDEN) return false;
  return true;
}

// "" = the description is valid; otherwise what is wrong with it (nothing is clamped)
inline std::string check(const Desc& d) {
  auto num = [](long long v) { return std::to_string(v); };
  if (d.n_states < 1 || d.n_states > MAX_STATES) return "n_states is " + num(d.n_states) + ", must be 1 .. " + num(MAX_STATES);
  if (d.n_classes < 1 || d.n_classes > MAX_CLASSES) return "n_classes is " + num(d.n_classes) + ", must be 1 .. " + num(MAX_CLASSES);
  if (d.n_states * d.n_classes > MAX_TRANS) return "n_states * n_classes is " + num(d.n_states * d.n_classes) + ", the limit is " + num(MAX_TRANS);
  if (d.vocab < 1 || d.vocab > MAX_VOCAB) return "vocab is " + num(d.vocab) + ", must be 1 .. " + num(MAX_VOCAB);
  if (d.start < 0 || d.start >= d.n_states) return "start state " + num(d.start) + " out of range";
  if (!d.token_class || !d.class_base || !d.trans) return "null array";
  std::vector<int> size(d.n_classes, 0);
  for (int t = 0; t < d.vocab; ++t) {
    if (d.token_class[t] >= d.n_classes) return "token " + num(t) + " has class " + num(d.token_class[t]) + ", n_classes is " + num(d.n_classes);
    ++size[d.token_class[t]];
  }
  for (int c = 0; c < d.n_classes; ++c) {
    const int b = d.class_base[c];
    if (b < -1 || b > d.vocab || (b >= 0 && size[c] > d.vocab - b)) return "class " + num(c) + ": base " + num(b) + " out of range";
    if (b >= 0) for (int t = b; t < b + size[c]; ++t)
      if (d.token_class[t] != c) return "ordinal class " + num(c) + " is not the contiguous id range " + num(b) + " .. " + num(b + size[c] - 1);
  }
  int max_set = 0;                                   // the largest class with a SET edge: reg < max_set always
  for (int s = 0; s < d.n_states; ++s) for (int c = 0; c < d.n_classes; ++c) {
    const uint16_t e = d.trans[s * d.n_classes + c];
    if (e == FORBIDDEN) continue;
    const std::string at = "edge (state " + num(s) + ", class " + num(c) + ")";
    if (e & ~(NEXT_MASK | SET | GE)) return at + ": reserved bits set";
    if ((e & NEXT_MASK) >= d.n_states) return at + ": next state " + num(e & NEXT_MASK) + " out of range";
    if ((e & (SET | GE)) && d.class_base[c] < 0) return at + ": SET / GE on a class that is not ordinal";
    if ((e & SET) && size[c] > max_set) max_set = size[c];
  }
  for (int s = 0; s < d.n_states; ++s) {
    if (is_end(d.trans, d.n_classes, s)) continue;
    bool live = false;                               // a token stays allowed whatever reg holds
    for (int c = 0; c < d.n_classes && !live; ++c) {
      const uint16_t e = d.trans[s * d.n_classes + c];
      live = e != FORBIDDEN && size[c] > 0 && (!(e & GE) || size[c] >= max_set);
    }
    if (!live) return "state " + num(s) + " can forbid every token: it needs an edge without GE on a non-empty class, or a GE edge on a class at least as large as every class with a SET edge";
  }
  return "";
}

// the device blob of a CHECKED description, as 32-bit words
inline std::vector<uint32_t> pack(const Desc& d) {
  Header h;
  const int nt = d.n_states * d.n_classes;
  h.n_states = d.n_states; h.n_classes = d.n_classes; h.start = d.start; h.vocab = d.vocab;
  h.off_base = (int)(sizeof(Header) / 4); h.off_trans = h.off_base + d.n_classes; h.off_class = h.off_trans + (nt + 1) / 2;
  h.words = h.off_class + (d.vocab + 3) / 4;
  std::vector<uint32_t> w((size_t)h.words, 0);
  memcpy(w.data(), &h, sizeof(h));
  memcpy(w.data() + h.off_base, d.class_base, (size_t)d.n_classes * 4);
  memcpy(w.data() + h.off_trans, d.trans, (size_t)nt * 2);
  memcpy(w.data() + h.off_class, d.token_class, (size_t)d.vocab);
  return w;
}
// a packed blob read back as a description (the arrays point into the blob)
inline Desc unpack(const uint32_t* blob) {
  Header h; memcpy(&h, blob, sizeof(h));
  return Desc{h.n_states, h.n_classes, h.start, h.vocab, reinterpret_cast<const uint8_t*>(blob + h.off_class), reinterpret_cast<const int32_t*>(blob + h.off_base),
              reinterpret_cast<const uint16_t*>(blob + h.off_trans)};
}

struct Walk { bool on; int state, reg; };
// the reference walk over the n generated ids
inline Walk walk(const Desc& d, const int32_t* ids, int n) {
  Walk w{n >= 0 && n <= HIST_CAP, d.start, 0};
  for (int i = 0; w.on && i < n; ++i) w.on = step(d.trans, d.n_classes, w.state, w.reg, pack_id(ids[i], d.vocab, d.token_class, d.class_base));
  return w;
}
// the row is masked at all: the walk is on and not in an END state
inline bool masks(const Desc& d, const Walk& w) { return w.on && !is_end(d.trans, d.n_classes, w.state); }
// id t survives the mask of a walk for which masks() holds
inline bool allowed(const Desc& d, const Walk& w, int t) {
  const int p = pack_id(t, d.vocab, d.token_class, d.class_base);
  return p != NO_CLASS && edge_allows(d.trans[w.state * d.n_classes + (p & 0xFF)], p >> 8, w.reg);
}

}  // namespace gvl_grammar
