// The argument checks of the admitting lookup, ONE function for tfra_table_find_or_insert (tfra_find_insert.hip) and for every
// descriptor of tfra_multi_find_or_insert (tfra_find_insert_many.hip), in the single call's order: the table, an empty batch, the
// buffers, the key count.  The message is without the entry point's prefix (Check, tfra_many.h).
#pragma once
#include "tfra_many.h"

static inline tfra::Check check_find_or_insert(const void* table, size_t n, const void* keys, const void* init_values) {
  if (!table) return tfra::refuse(TFRA_ERR_INVALID, "null table");
  if (n == 0) return tfra::nothing_to_do();
  if (!keys || !init_values) return tfra::refuse(TFRA_ERR_INVALID, "null buffer");
  if (n >= (1ULL << 31)) return tfra::refuse(TFRA_ERR_INVALID, "more than 2^31-1 keys per call");
  return tfra::Check{};
}
