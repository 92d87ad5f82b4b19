// A caller's row mask sliced to one shard (tostore_amd/csrc/tsh_host_sync.h slice_mask, mask_kept_rows, popcount_words,
// list_mask_bits) and put back (unslice_mask) on every row base 0..71 and a few large ones, every shard length 1..200 and a few around 4096 and
// 65536, with the shard's range zero, all ones or random and the bits around it set (or, for the last kind, clear).
// argv[1]: the random range content (bit i of the file = bit i of the range), argv[2]: where the results go -- one
// record per case, int64 {row_base, rows, kind, popcount, kept, listed, sum of ids, sum of (position + 1) * id} then
// the ceil(rows / 64) + 1 words slice_mask wrote.  tests/test_host_mask.py holds them to NumPy.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tostore_amd/csrc/tsh_host_sync.h"

// unslice_mask, slice_mask's other half: the sliced words of [base, base + rows) put back into a zeroed bitmap of
// (base + rows + 7) / 8 + 1 bytes between canaries must give the source's bits inside the range and nothing outside it;
// then an adjacent range of 37 ones into the same bitmap, grown as a handle's is, must leave every bit of the first
// (the shared byte is or-ed).  Returns what is wrong, or nullptr.
static const char *unslice_check(int64_t base, int64_t rows, const uint8_t *src, const uint64_t *words) {
  const size_t PAD = 16;
  const uint8_t CAN = 0xC5;
  const int64_t rows2 = 37, end = base + rows, end2 = end + rows2;
  const size_t n1 = (size_t)((end + 7) / 8) + 1, n2 = (size_t)((end2 + 7) / 8) + 1;
  static std::vector<uint8_t> buf;
  buf.assign(PAD + n2 + PAD, CAN);
  uint8_t *bits = buf.data() + PAD;
  auto bit = [](const uint8_t *b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; };
  // the bits of [0, n_bits) against: zero below `base`, the source in the first range, `second` in the second, zero after
  auto holds = [&](size_t n_bytes, int second) {
    for (int64_t i = 0; i < (int64_t)n_bytes * 8; ++i) {
      const int want = i < base ? 0 : i < end ? bit(src, i) : i < end2 ? second : 0;
      if (bit(bits, i) != want) return false;
    }
    return true;
  };
  auto canaries = [&](size_t n_bytes) {
    for (size_t i = 0; i < PAD; ++i)
      if (buf[i] != CAN) return false;
    for (size_t i = PAD + n_bytes; i < buf.size(); ++i)
      if (buf[i] != CAN) return false;
    return true;
  };
  memset(bits, 0, n1);
  tsh::unslice_mask(base, rows, words, bits);
  if (!canaries(n1)) return "wrote outside the bitmap";
  if (!holds(n1, 0)) return "the bitmap is not the source's range and zero around it";
  memset(bits + n1, 0, n2 - n1);
  const uint64_t ones = (1ull << rows2) - 1;
  tsh::unslice_mask(end, rows2, &ones, bits);
  if (!canaries(n2)) return "the adjacent range wrote outside the bitmap";
  if (!holds(n2, 1)) return "the adjacent range did not leave the first as it was";
  return nullptr;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<uint8_t> rnd;
  {
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int c;
    while ((c = fgetc(f)) != EOF) rnd.push_back((uint8_t)c);
    fclose(f);
  }
  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  std::vector<int64_t> bases, lens;
  for (int64_t b = 0; b < 72; ++b) bases.push_back(b);
  for (int64_t b : {12347ll, 23360ll, (1ll << 20) + 3}) bases.push_back(b);
  for (int64_t r = 1; r <= 200; ++r) lens.push_back(r);
  for (int64_t r : {4095ll, 4096ll, 4097ll, 65535ll, 65536ll, 65537ll}) lens.push_back(r);
  if ((int64_t)rnd.size() * 8 < 65537) return 2;
  const uint32_t CANARY = 0xC0FFEE11u;
  long cases = 0;
  for (int64_t base : bases)
    for (int64_t rows : lens)
      for (int kind = 0; kind < 4; ++kind) {
        // kind 0: range zero, 1: range all ones, 2: range random -- each with every bit around it set; 3: range
        // random, nothing around it.  The bitmap ends a few bytes past the range: bits after it exist and are set.
        const uint8_t around = kind == 3 ? 0x00 : 0xFF;
        std::vector<uint8_t> g((size_t)((base + rows) / 8 + 9), around);
        for (int64_t i = 0; i < rows; ++i) {
          const int bit = kind == 0 ? 0 : kind == 1 ? 1 : (rnd[(size_t)(i >> 3)] >> (i & 7)) & 1;
          const int64_t j = base + i;
          if (bit) g[(size_t)(j >> 3)] |= (uint8_t)(1u << (j & 7));
          else g[(size_t)(j >> 3)] &= (uint8_t)~(1u << (j & 7));
        }
        const int32_t n_tiles = (int32_t)((rows + 63) / 64);
        const int64_t n_words = n_tiles + 1;  // (one more than the shard needs: slice_mask clears all it is given)
        std::vector<uint64_t> words((size_t)n_words, 0xA5A5A5A5A5A5A5A5ull);
        tsh::slice_mask(base, rows, g.data(), words.data(), n_words);
        const int64_t pop = tsh::popcount_words(words.data(), (size_t)n_words);
        const int64_t kept = tsh::mask_kept_rows(base, rows, g.data());
        std::vector<uint32_t> list((size_t)pop + 4 + 64, CANARY);
        const size_t listed = tsh::list_mask_bits(words.data(), n_tiles, pop, list.data());
        uint64_t sum = 0, wsum = 0;
        for (size_t j = 0; j < listed && j < list.size(); ++j) {
          sum += list[j];
          wsum += (uint64_t)(j + 1) * list[j];
        }
        for (size_t j = listed + 4; j < list.size(); ++j)
          if (list[j] != CANARY) {
            fprintf(stderr, "list_mask_bits wrote past its count + 4: base %lld rows %lld kind %d\n", (long long)base,
                    (long long)rows, kind);
            return 1;
          }
        if (const char *what = unslice_check(base, rows, g.data(), words.data())) {
          fprintf(stderr, "unslice_mask: %s: base %lld rows %lld kind %d\n", what, (long long)base, (long long)rows, kind);
          return 1;
        }
        const int64_t rec[8] = {base, rows, kind, pop, kept, (int64_t)listed, (int64_t)sum, (int64_t)wsum};
        fwrite(rec, sizeof(rec), 1, out);
        fwrite(words.data(), 8, (size_t)n_words, out);
        ++cases;
      }
  fclose(out);
  printf("ok %ld cases\n", cases);
  return 0;
}
