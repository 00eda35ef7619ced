// Host stage of leading-line detection (lines_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace fe {
// map [h][w]: 2 = edge, 0 = edge if 8-connected to a 2, 1 = not an edge -> in place 255 / 0
void canny_hysteresis(uint8_t* map, int h, int w);
// edges [h][w] (non-zero = edge) -> first max_lines segments (x1,y1,x2,y2) into `lines`; returns the number found (may exceed max_lines)
int hough_lines_p(const uint8_t* edges, int h, int w, int threshold, int min_len, int max_gap, int max_lines, int* lines);
// maps [n][h][w] -> edges in place and, when lines != nullptr, lines [n][max_lines][4] + counts [n]; one image per host thread
void lines_host_stage(uint8_t* maps, int n, int h, int w, int threshold, int min_len, int max_gap, int max_lines, int* lines, int* counts, int threads);
// the same for n images of their own sizes: image i lies at maps + offsets[i] and is hw[2 i] x hw[2 i + 1] with min_len[i]; lines
// [n][max_lines][4] + counts [n]. At most min(threads, 16) host threads, which take the images largest first from a shared cursor.
void lines_host_stage_mixed(uint8_t* maps, const size_t* offsets, const int32_t* hw, int n, int threshold, const int32_t* min_len, int max_gap,
                            int max_lines, int* lines, int* counts, int threads);
}  // namespace fe
