// kernel instantiations for drive law KB_DRIVE_VELOCITY: without objects, with polygon objects, and the num_bots == 1024
// specialisations (the benchmark shapes)
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_VELOCITY && v.poly; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
