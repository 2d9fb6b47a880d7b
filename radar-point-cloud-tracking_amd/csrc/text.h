// The rpt:: functions that text.hip (floats -> text rows) and ply_parse.hip (text rows ->
// floats) define, declared once.  Included by both files, so every definition is compiled against
// its declaration, and by abi.cpp (the extern "C" surface).
#pragma once
#include "common.h"

namespace rpt {

// ---- text.hip: rows of layout (RPT_TEXT_*) from the columns x, y, z and the layout's tail
// row_offsets ([n + 1], device): each row's byte offset, the total last; *total_host: the total;
// *n_bad_host: rows outside the layout's domain (length 0).  Synchronises.
int32_t text_rows_size(int32_t layout, const float* x, const float* y, const float* z,
                       const void* tail, int64_t n, int64_t* row_offsets, int64_t* total_host,
                       int64_t* n_bad_host, hipStream_t st);
// the rows at row_offsets (from text_rows_size over the same arguments) into out[out_bytes]
int32_t text_rows_write(int32_t layout, const float* x, const float* y, const float* z,
                        const void* tail, int64_t n, const int64_t* row_offsets, uint8_t* out,
                        int64_t out_bytes, hipStream_t st);

// ---- ply_parse.hip: ASCII rows of decimal numbers -> float32 columns
// bytes of text one block of text_rows_index takes
int64_t text_tile_bytes();
// row_start ([n_rows + 1], device): byte offset of every line of text[nbytes], lines beyond the
// text's own left past nbytes; *lines_found_host: the text's lines; *n_bad_host: bytes no vertex
// row may hold.  Synchronises.
int32_t text_rows_index(const uint8_t* text, int64_t nbytes, int64_t n_rows, uint32_t* row_start,
                        int64_t* lines_found_host, int64_t* n_bad_host, hipStream_t st);
// out[c * n_rows + i] = token c of row i; *n_bad_host: rows with another token count than n_cols,
// a token outside parse32's domain or too many bytes (the caller then discards out).  Synchronises.
int32_t text_rows_parse(const uint8_t* text, int64_t nbytes, const uint32_t* row_start,
                        int64_t n_rows, int32_t n_cols, float* out, int64_t* n_bad_host,
                        hipStream_t st);

}  // namespace rpt
