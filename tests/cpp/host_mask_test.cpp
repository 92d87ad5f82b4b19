// A caller's row mask sliced to one shard (tostore_amd/csrc/tsh_host_sync.h slice_mask, mask_kept_rows, popcount_words,
// list_mask_bits) on every row base 0..71 and a few large ones, every shard length 1..200 and a few around 4096 and
// 65536, with the shard's range zero, all ones or random and the bits around it set (or, for the last kind, clear).
// argv[1]: the random range content (bit i of the file = bit i of the range), argv[2]: where the results go -- one
// record per case, int64 {row_base, rows, kind, popcount, kept, listed, sum of ids, sum of (position + 1) * id} then
// the ceil(rows / 64) + 1 words slice_mask wrote.  tests/test_host_mask.py holds them to NumPy.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tostore_amd/csrc/tsh_host_sync.h"

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
        const int64_t rec[8] = {base, rows, kind, pop, kept, (int64_t)listed, (int64_t)sum, (int64_t)wsum};
        fwrite(rec, sizeof(rec), 1, out);
        fwrite(words.data(), 8, (size_t)n_words, out);
        ++cases;
      }
  fclose(out);
  printf("ok %ld cases\n", cases);
  return 0;
}
