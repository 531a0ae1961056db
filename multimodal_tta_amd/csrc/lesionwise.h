// What the lesion-wise Dice pass (lesionwise.hip) and the lesion-wise HD95 pass (lesionwise_hd95.hip) share: the limits and
// the layout of the scratch that mmtta_lesionwise_scores leaves behind, which the HD95 pass only reads.
#pragma once
#include "components.h"

namespace mmtta {

static inline size_t lw_align(size_t v) { return (v + 255) & ~(size_t)255; }

static inline bool lw_extent_ok(int64_t n_masks, int64_t d, int64_t h, int64_t w) {
  if (n_masks < 1 || n_masks > 65535 || d < 1 || h < 1 || w < 1) return false;
  if (d > CC_MAX_V || h > CC_MAX_V || w > CC_MAX_V || d * h > CC_MAX_V || d * h * w > CC_MAX_V) return false;
  return n_masks * ((d * h * w + 255) / 256) <= CC_MAX_BLOCKS;
}

// slots of one mask's pair table (see the top of lesionwise.hip) and their log2
static inline unsigned long long lw_table_slots(int64_t d, int64_t h, int64_t w, int& logcap) {
  const unsigned long long pairs = (unsigned long long)((d + 1) / 2) * (unsigned long long)((h + 1) / 2) * (unsigned long long)((w + 1) / 2);
  unsigned long long cap = 2;
  logcap = 1;
  while (cap < 2 * pairs) { cap <<= 1; ++logcap; }
  return cap;
}

struct LwLayout {
  size_t head, zero_bytes, sizeP, pg, own, inter, matched, LG, LP, gd, table, total;
};

// [header | sizeP | pg | own | inter | matched] are zeroed by one memset; then the labels, Gd and the pair tables
static inline LwLayout lw_layout(int64_t M, int64_t V, unsigned long long cap) {
  LwLayout l;
  const size_t mv = (size_t)M * (size_t)V;
  l.head = lw_align((size_t)M * 32);
  size_t o = l.head;
  l.sizeP = o; o += lw_align(mv * 4);
  l.pg = o; o += lw_align(mv * 4);
  l.own = o; o += lw_align(mv * 4);
  l.inter = o; o += lw_align(mv * 4);
  l.matched = o; o += lw_align(mv);
  l.zero_bytes = o;
  l.LG = o; o += lw_align(mv * 4);
  l.LP = o; o += lw_align(mv * 4);
  l.gd = o; o += lw_align(mv);
  l.table = o; o += lw_align((size_t)M * (size_t)cap * 8);
  l.total = o;
  return l;
}

}  // namespace mmtta
