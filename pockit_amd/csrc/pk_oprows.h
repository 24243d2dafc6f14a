// pk_oprows.h -- private to the units whose kernels walk the row blocks of an operator (pk_ops.cpp: the products; pk_reduce.cpp:
// the reductions over a row's entries): where the 256 terms of a block lie in LDS.  Nothing else is shared: the terms, the
// association and the rounding of every result are each unit's own.
#ifndef PK_OPROWS_H
#define PK_OPROWS_H

#include "pk_libkernel.h"

// LDS slot of product i: one slot of padding behind every 32.  ds_read_b64 serves a wave as two halves of 32 lanes over
// 64 banks of 4 bytes, i.e. 32 doubles per cycle: lane r of the row sums reads slot (start of row r) + k, a stride of the
// row length -- 2, 4, 8 ... doubles for rows of equal even length would be 2-, 4-, 8-way conflicts; with the padding lanes
// r and r + 32 / len land one bank pair further and the half-wave is conflict-free for every power-of-two length up to 32.
#define PK_OP_LDS (PK_BLOCK + PK_BLOCK / 32)
PK_LIB_FN int op_slot(int i) { return i + (i >> 5); }

#endif  // PK_OPROWS_H
