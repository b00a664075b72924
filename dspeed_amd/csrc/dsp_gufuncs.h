// dsp_gufuncs.h -- the two things the single-processor entry points (dsp_gufuncs.cpp) need from the HIP side of the library.  That file
// is a pure client of dsp_chain_create / execute / check / destroy and includes no HIP header, so that it is also compiled for the CPU with
// -fsanitize=address,undefined against stand-ins (tests/gufunc_programs.cpp); dsp_host.cpp defines the real ones.  Internal header.
#pragma once
#include <stddef.h>

// the device the calling thread has selected: part of the key a cached chain is found by
int dsp_gufunc_current_device();
// device -> host copy of a few bytes through the library's page-locked staging buffer (the runtime is never handed heap memory);
// DSP_OK, or DSP_ERR_HIP with the text in dsp_last_error()
int dsp_gufunc_read_back(void* host, const void* dev, size_t bytes);
