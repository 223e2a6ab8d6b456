// The library's internal status values (capi.cpp maps them onto the MG_* codes of include/mantagpu.h).
#pragma once
namespace mg {
enum { MG_OK = 0, MG_ERR_ARG = 1, MG_ERR_HIP = 2, MG_ERR_OOM = 3, MG_ERR_DOMAIN = 4, MG_ERR_STATE = 5 };
}
