// kernel instantiations for drive law KB_DRIVE_ACCEL: without objects and with polygon objects
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_ACCEL && v.poly; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
