/* Stand-alone driver of the CPU reference (tests/klt_ref/klt_ref.c) for a sanitizer build: reads one
 * problem from a file, tracks it, and prints every output word in hex, one point per line.
 * File: int32 rows, cols, n, levels, bh, bw, max_iterations, has_guess; float max_bidirectional_error;
 * img0 [rows][cols] u8; img1; pts0 [n][2] float; guess [n][2] float when has_guess. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { uint8_t status, stop, iterations, levels_skipped; float bidir_error; } klt_info;
long klt_ref_layout(int rows, int cols, int levels, long* off);
void klt_ref_pyramid(const uint8_t* img, int rows, int cols, int levels, uint8_t* out);
void klt_ref_track(const uint8_t* pyr0, const uint8_t* pyr1, int rows, int cols, const float* pts0, const float* guess, int n,
                   int levels, int bh, int bw, int max_it, float max_bidir, float* pts1, uint8_t* valid, float* scores, klt_info* info,
                   uint8_t* level_codes);

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: klt_ref_main problem.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[8];
    float max_bidir;
    if (fread(h, 4, 8, f) != 8 || fread(&max_bidir, 4, 1, f) != 1) return 2;
    const int rows = h[0], cols = h[1], n = h[2], levels = h[3], bh = h[4], bw = h[5], max_it = h[6], has_guess = h[7];
    if (rows < 1 || cols < 1 || rows > 4096 || cols > 4096 || n < 0 || n > 100000 || levels < 1 || levels > 6) return 2;
    const size_t px = (size_t)rows * cols;
    const long total = klt_ref_layout(rows, cols, levels, 0);
    uint8_t* img = malloc(2 * px);
    uint8_t* pyr0 = malloc((size_t)total);
    uint8_t* pyr1 = malloc((size_t)total);
    float* pts0 = malloc(sizeof(float) * 2 * (size_t)(n + 1));
    float* guess = malloc(sizeof(float) * 2 * (size_t)(n + 1));
    float* pts1 = malloc(sizeof(float) * 2 * (size_t)(n + 1));
    float* scores = malloc(sizeof(float) * (size_t)(n + 1));
    uint8_t* valid = malloc((size_t)n + 1);
    klt_info* info = malloc(sizeof(klt_info) * (size_t)(n + 1));
    if (fread(img, 1, 2 * px, f) != 2 * px || fread(pts0, 8, (size_t)n, f) != (size_t)n) return 2;
    if (has_guess && fread(guess, 8, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    klt_ref_pyramid(img, rows, cols, levels, pyr0);
    klt_ref_pyramid(img + px, rows, cols, levels, pyr1);
    klt_ref_track(pyr0, pyr1, rows, cols, pts0, has_guess ? guess : 0, n, levels, bh, bw, max_it, max_bidir, pts1, valid, scores, info, 0);
    for (int i = 0; i < n; ++i)
        printf("%08x %08x %d %08x %d %d %d %d %08x\n", bits(pts1[2 * i]), bits(pts1[2 * i + 1]), valid[i], bits(scores[i]), info[i].status,
               info[i].stop, info[i].iterations, info[i].levels_skipped, bits(info[i].bidir_error));
    free(img); free(pyr0); free(pyr1); free(pts0); free(guess); free(pts1); free(scores); free(valid); free(info);
    return 0;
}
