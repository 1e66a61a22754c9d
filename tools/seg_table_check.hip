// Stand-alone host check of bt_segments.h's table builders, meant for AddressSanitizer / UBSan (no GPU, not loaded into Python):
//   make -C bayesian_torch_amd/csrc segcheck
// Over the launch sweep's lengths and caps (tools/record_seg_launches.py): first_block is non-decreasing, starts at 0, its last entry
// is the returned grid, no segment exceeds its cap, a refusal leaves its text; seg_layers sets bit 0 and refuses a decreasing list.
#include <string.h>

#include <vector>

#include "../bayesian_torch_amd/csrc/bt_segments.h"

namespace bt {
static char g_err[512];
int set_error(int code, const char* msg) {
  strncpy(g_err, msg, sizeof(g_err) - 1);
  return code;
}
}  // namespace bt

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #c);           \
      ++failures;                                             \
    }                                                         \
  } while (0)

static void partition_case(const std::vector<int64_t>& work, int per_block, long long cap, int slots) {
  // the table sits in a heap block of exactly its size, so that a write past first_block[nseg] or n[] is the sanitizer's to see
  bt::SegTable* t = new bt::SegTable();
  const int nseg = (int)work.size();
  bt::g_err[0] = 0;
  const int blocks = bt::seg_partition(*t, nseg, work.data(), per_block, cap, slots, "check");
  long long want = 0;
  bool over = false;
  for (int i = 0; i < nseg; ++i) {
    long long nb = (work[i] + per_block - 1) / per_block;
    if (cap && nb > cap) nb = cap;
    want += nb;
    over = over || want > (slots ? slots : 0x7FFFFFFFll);
  }
  if (over) {
    CHECK(blocks == BT_ERR_UNSUPPORTED);
    CHECK(strstr(bt::g_err, slots ? "check: too many blocks for the workspace" : "check: too many elements for one launch") != nullptr);
  } else {
    CHECK(blocks == (int)want);
    CHECK(t->nseg == nseg && t->first_block[0] == 0 && t->first_block[nseg] == blocks);
    for (int i = 0; i < nseg; ++i) {
      const int nb = t->first_block[i + 1] - t->first_block[i];
      CHECK(nb >= 1 && (!cap || nb <= cap));
      CHECK((long long)nb == (cap && (work[i] + per_block - 1) / per_block > cap ? cap : (work[i] + per_block - 1) / per_block));
    }
  }
  delete t;
}

int main() {
  const int64_t lens[] = {1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193};
  const int counts[] = {1, 2, 3, 63, 64};
  struct Rule { int per_block; long long cap; int slots; };
  const Rule rules[] = {{4096, 1024, bt::kMaxSlots}, {4096, 2048, bt::kMaxSlots}, {1024, 0, 0}, {4096, 128, 0}, {4096, bt::kMaxSlots / 64, 0}, {1, 256, 0}};
  for (const Rule& r : rules) {
    for (int n : counts)
      for (int shift = 0; shift < 13; ++shift) {
        std::vector<int64_t> w;
        for (int i = 0; i < n; ++i) w.push_back(lens[(i + shift) % 13]);
        partition_case(w, r.per_block, r.cap, r.slots);
      }
    if (r.cap) {   // the cap, one element and one block past it, alone and in 64 segments (past the workspace's slots where there is a limit)
      const int64_t at = r.cap * r.per_block;
      for (int64_t ln : {at - 1, at, at + 1, at + r.per_block + 1})
        for (int n : {1, 3, 7, 8, 64}) partition_case(std::vector<int64_t>(n, ln), r.per_block, r.cap, r.slots);
    } else {       // the grid's 2^31 - 1 blocks and one past them
      const int64_t top = 0x7FFFFFFFll * r.per_block;
      partition_case({top}, r.per_block, 0, 0);
      partition_case({top + 1}, r.per_block, 0, 0);
      partition_case({top - r.per_block, 2 * (int64_t)r.per_block}, r.per_block, 0, 0);
      partition_case(std::vector<int64_t>(64, top), r.per_block, 0, 0);
    }
  }
  bt::SegTable* t = new bt::SegTable();
  std::vector<int32_t> lay(64);
  CHECK(bt::seg_layers(*t, 64, nullptr, "check") == BT_OK && t->new_layer == ~0ull);
  for (int i = 0; i < 64; ++i) lay[i] = 5;
  CHECK(bt::seg_layers(*t, 64, lay.data(), "check") == BT_OK && t->new_layer == 1ull);
  for (int i = 0; i < 64; ++i) lay[i] = i / 2;
  CHECK(bt::seg_layers(*t, 64, lay.data(), "check") == BT_OK && t->new_layer == 0x5555555555555555ull);
  CHECK(bt::seg_layers(*t, 1, lay.data(), "check") == BT_OK && t->new_layer == 1ull);
  lay[63] = 0;
  CHECK(bt::seg_layers(*t, 64, lay.data(), "check") == BT_ERR_BAD_ARG && strstr(bt::g_err, "check: layer_of_segment must be non-decreasing"));
  delete t;
  printf(failures ? "seg_table_check: %d FAILED\n" : "seg_table_check: ok\n", failures);
  return failures ? 1 : 0;
}
