// Our own stand-in: the reference's include/read_arrays.hpp includes this sdsl header but uses none of its names.
#ifndef MMT_SDSL_SHIM_INT_VECTOR_HPP
#define MMT_SDSL_SHIM_INT_VECTOR_HPP
#include "io.hpp"
#endif
