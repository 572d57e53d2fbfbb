// The grouped launch form of attn_w64_kernel (AttnGroupArgs, kernels.h): the same block body, w64_block<SPLIT, true> of attn_w64.hip,
// behind a kernel that takes the second argument struct.  The instantiations live in a translation unit of their own so that
// attn_w64.hip compiles to the two kernels it always had (the ISA audit counts them, and an ungrouped launch runs what it ran before);
// tests/test_isa_audit_groups.py audits this one the same way: the body names a[0:255] literally here too.
#define MMPL_ATTN_W64_GROUPS_TU 1
#include "attn_w64.hip"

const void* mmpl_attention_w64_groups_symbol(int split) {
  return split ? reinterpret_cast<const void*>(attn_w64_groups_kernel<true>) : reinterpret_cast<const void*>(attn_w64_groups_kernel<false>);
}
void mmpl_launch_attention_w64_groups(const AttnGroupArgs& ga, int blocks, int local_base, int sp, bool split, hipStream_t s) {
  if (split) hipLaunchKernelGGL(attn_w64_groups_kernel<true>, dim3(blocks), dim3(256), W64_SMEM, s, ga, local_base, sp);
  else hipLaunchKernelGGL(attn_w64_groups_kernel<false>, dim3(blocks), dim3(256), W64_SMEM, s, ga, local_base, sp);
}
