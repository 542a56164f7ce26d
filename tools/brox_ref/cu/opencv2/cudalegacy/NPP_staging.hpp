/* tools/brox_ref/cu -- TEST INFRASTRUCTURE.  Stand-in for the header of this name in modules/cudalegacy/include: see brox_ncv_standin.hpp. */
#include "brox_ncv_standin.hpp"
