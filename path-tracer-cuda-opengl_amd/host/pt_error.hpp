// pt_error.hpp — thread-local last-error string behind pt_last_error().
// Replaces checkCudaErrors' print + cudaDeviceReset + exit(99) (utils/cuda_check.h:8-17):
// the library never exits the process; it returns a status code and records a message.
#pragma once
#include <string>

namespace pt {
// One definition (pt_host.cpp) for every translation unit: an inline function's local static is
// mangled differently by the host compiler and by hipcc, which gave the HIP units a string of
// their own that pt_last_error() never read.
std::string& lastError();
inline int fail(int code, const std::string& msg) {
    lastError() = msg;
    return code;
}
}  // namespace pt
