// The grouped launch form of attn_w64_kernel (AttnGroupArgs, kernels.h): the same block body, w64_block<SPLIT, true> of attn_w64.hip,
// behind a kernel that takes the second argument struct.  The instantiations live in a translation unit of their own so that
// attn_w64.hip compiles to the two kernels it always had (the ISA audit counts them, and an ungrouped launch runs what it ran before);
// tests/test_isa_audit_groups.py audits this one the same way: the body names a[0:255] literally here too.
#define MMPL_ATTN_W64_GROUPS_TU 1
#include "attn_w64.hip"

template <> AttnW64Kernels<AttnGroupArgs> mmpl_attention_w64_kernels<AttnGroupArgs>() {
  return {attn_w64_groups_kernel<true>, attn_w64_groups_kernel<false>};
}
