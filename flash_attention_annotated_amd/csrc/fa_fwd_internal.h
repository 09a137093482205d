// fa_fwd_internal.h — host helpers of fa_fwd_api.hip that fa_fwd_kv8_api.hip and fa_fwd_qv8_api.hip call (not part of the C-ABI).  They keep the
// split-KV heuristic and the last-plan text of fa_fwd_last_plan_name() in fa_fwd_api.hip.
#pragma once

#include "fa_fwd.h"

namespace fa {

// Parts of the key range for the pk work shape (blocks of 128 packed rows per kv head, 4 waves; split_plan of fa_fwd_api.hip):
// num_splits 1 = off, N > 1 = N (clamped to the key blocks), 0 = the heuristic.  Counted from shapes only.  `p` is 16-bit.
int fwd_pk_split_count(const fa_fwd_params *p);

// The same for the qv work shape (blocks of 32 packed rows per kv head, one workgroup per CU; split_plan_qv of fa_fwd_api.hip):
// what the 16-bit qv call of the same shape is split into.  Reads the shape fields and num_splits only.
int fwd_qv_split_count(const fa_fwd_params *p);

// What fa_fwd_last_plan_name() answers for the calling thread until its next fa_fwd / fa_fwd_sink / fa_fwd_block_sparse;
// NULL or "" = nothing.
void fwd_set_last_plan_text(const char *text);

// compute units of the current device (cached per device ordinal)
int fwd_device_cus();

}  // namespace fa
