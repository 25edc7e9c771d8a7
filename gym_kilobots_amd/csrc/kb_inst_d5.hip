// kernel instantiations for KB_DRIVE_MIXED: any mix of the five drive laws in one env, one-wave workgroups (256 VGPRs:
// no spills), the code path with per-body masses
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_MIXED && v.tier == 1; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
