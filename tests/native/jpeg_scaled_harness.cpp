// Host harness for the scaled decode of facet_amd/csrc/jpeg_dec_core.h (decode_host_scaled): the reduced transforms, the per-component
// plane layout and the upsampling choice, under AddressSanitizer + UBSan (tests/test_jpeg_scaled_host.py).
//   in:  int32 n, bgr, apply_orientation, flags; n x { int32 scale; uint32 len; len bytes }
//   out: n x { int32 status, oh, ow; oh * ow * 3 bytes when status == 0 }
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
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (int i = 0; i < hdr[0]; ++i) {
    int32_t scale;
    uint32_t len;
    if (fread(&scale, 4, 1, f) != 1 || fread(&len, 4, 1, f) != 1) return 2;
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return 2;
    // exactly the file: the parser must not read past it
    uint8_t* file = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(file, 1, len, f) != len) return 2;
    Parsed P;
    parse(file, len, P, hdr[3]);
    int32_t res[3] = {P.status, 0, 0};
    std::vector<uint8_t> out;
    if (P.status == ST_OK) {
      // the decoder reads aligned 16-byte chunks: the buffer is padded to a multiple of 16 and no further
      const size_t padded = ((size_t)len + 15) & ~(size_t)15;
      uint8_t* buf = (uint8_t*)aligned_alloc(16, padded);
      memset(buf, 0, padded);
      memcpy(buf, file, len);
      const bool swap = hdr[2] && P.orientation >= 5;
      const int sh = (P.height + scale - 1) / scale, sw = (P.width + scale - 1) / scale;
      res[1] = swap ? sw : sh; res[2] = swap ? sh : sw;
      out.resize((size_t)res[1] * res[2] * 3);      // exactly the scaled image: a write past it is a report
      res[0] = decode_host_scaled(P, buf, scale, hdr[1], hdr[2], out.data());
      free(buf);
    }
    free(file);
    fwrite(res, 4, 3, o);
    if (res[0] == ST_OK) fwrite(out.data(), 1, out.size(), o);
  }
  fclose(o);
  fclose(f);
  return 0;
}
