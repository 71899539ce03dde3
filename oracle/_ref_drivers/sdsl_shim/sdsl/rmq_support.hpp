// Our own stand-in: the reference's include/read_arrays.hpp includes this sdsl header but uses none of its names.
#ifndef MMT_SDSL_SHIM_RMQ_SUPPORT_HPP
#define MMT_SDSL_SHIM_RMQ_SUPPORT_HPP
#include "io.hpp"
#endif
