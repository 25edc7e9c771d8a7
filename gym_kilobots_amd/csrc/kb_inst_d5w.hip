// kernel instantiations for KB_DRIVE_MIXED beyond 128 kilobots: the full workgroup at 256 VGPRs (two waves per SIMD:
// one env per CU, no spills)
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_MIXED && v.tier == 3; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
