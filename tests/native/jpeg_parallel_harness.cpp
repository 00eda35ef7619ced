// Host harness for the parallel entropy decode of facet_amd/csrc/jpeg_dec_core.h: steps 1 to 4 of the self-synchronising decoder with
// the lanes as loops, next to the serial decode_host of the same file, both under AddressSanitizer + UBSan
// (tests/test_jpeg_parallel_host.py).
//   in:  int32 n, bgr, apply_orientation, S; n x { uint32 len; len bytes }
//   out: n x { int32 status, oh, ow, serial status, rounds, redone, parallel segments, subsequences;
//              oh * ow * 3 bytes when status == 0; oh * ow * 3 bytes of decode_host when serial status == 0 }
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_dec_core.h"

using namespace fe::jpegdec;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4) return 2;
  const uint32_t S = (uint32_t)hdr[3];
  if (S < 16 || (S & (S - 1))) return 2;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (int i = 0; i < hdr[0]; ++i) {
    uint32_t len;
    if (fread(&len, 4, 1, f) != 1) return 2;
    uint8_t* file = (uint8_t*)malloc(len ? len : 1);         // exactly the file: the parser must not read past it
    if (len && fread(file, 1, len, f) != len) return 2;
    Parsed P;
    parse(file, len, P);
    int32_t res[8] = {P.status, 0, 0, P.status, 0, 0, 0, 0};
    std::vector<uint8_t> out, ref;
    if (P.status == ST_OK) {
      const size_t padded = ((size_t)len + 15) & ~(size_t)15;      // aligned 16-byte chunks and no further
      uint8_t* buf = (uint8_t*)aligned_alloc(16, padded);
      memset(buf, 0, padded);
      memcpy(buf, file, len);
      const bool swap = hdr[2] && P.orientation >= 5;
      res[1] = swap ? P.width : P.height; res[2] = swap ? P.height : P.width;
      out.resize((size_t)res[1] * res[2] * 3);
      ref.resize(out.size());
      ParallelStats ps;
      res[0] = decode_host_parallel(P, buf, S, hdr[1], hdr[2], out.data(), ps);
      res[3] = decode_host(P, buf, hdr[1], hdr[2], ref.data());
      res[4] = (int32_t)ps.rounds; res[5] = (int32_t)ps.redone; res[6] = (int32_t)ps.segments; res[7] = (int32_t)ps.subsequences;
      free(buf);
    }
    free(file);
    fwrite(res, 4, 8, o);
    if (res[0] == ST_OK) fwrite(out.data(), 1, out.size(), o);
    if (res[3] == ST_OK) fwrite(ref.data(), 1, ref.size(), o);
  }
  fclose(o);
  fclose(f);
  return 0;
}
