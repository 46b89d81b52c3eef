/*
 * imgrec_resize.h — C ABI of the 8-bit LANCZOS resize (Pillow's Image.resize(size, LANCZOS)).
 *
 * Restates Pillow's Resample.c for 8 bits per channel with box = the whole image, bit for bit:
 * per axis a table of integer weights (22 fractional bits) built on the host in double with
 * libm's sin, a horizontal pass over every input row whose result is rounded to uint8, then a
 * vertical pass over those bytes.  A pass whose input and output lengths are equal is skipped;
 * when both are, the result is a copy.  Channels are independent.  One output byte is
 * clamp((2^21 + sum_j px[xmin + j] * k[j]) >> 22, 0, 255) in int32 arithmetic.  DESIGN.md,
 * "LANCZOS resize", has the table's formulas.
 *
 * Images are interleaved 8-bit (HWC), channels = 3 (RGB) or 1 (L).  Sizes are (height, width)
 * here; the Python wrappers take Pillow's (width, height).
 */
#ifndef IMGREC_RESIZE_H
#define IMGREC_RESIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RESIZE_U8_HWC 0  /* n x out_h x out_w x channels bytes */
#define RESIZE_F32_CHW 1 /* n x channels x out_h x out_w floats, (float)byte / 255.0f */

/* One image on the host, plain C++ with no GPU call: pixels h x w x channels -> out_u8
 * out_h x out_w x channels.  The library's own CPU statement of the arithmetic. */
int resize_lanczos_host(const uint8_t* pixels, int h, int w, int channels, int out_h, int out_w,
                        uint8_t* out_u8);

/* A ragged batch on the device.  Image i is host_heights[i] x host_widths[i] x channels bytes at
 * dev_pixels + host_offsets[i] (any alignment); the three arrays are host memory and are read
 * before the call returns.  dev_out receives the n results in `format`.  Enqueued on `stream`
 * (hipStream_t, NULL = default stream), no sync; calls on different streams are ordered.  An
 * image's result does not depend on the rest of the batch. */
int resize_lanczos_device(const uint8_t* dev_pixels, const int64_t* host_offsets,
                          const int32_t* host_heights, const int32_t* host_widths, int64_t n,
                          int channels, int out_h, int out_w, int format, void* dev_out,
                          void* stream);

/* Same error-string convention as knn_last_error(). */
const char* resize_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* IMGREC_RESIZE_H */
