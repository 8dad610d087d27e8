// f0_override.h -- what the engine and the kernels of f0_override.hip.h share; no kernel is defined here
#pragma once

namespace rvc {

constexpr int F0_OV_ROWS = 1024;       // an override row buffer holds at most this many rows per stream (the longest f0 window)
constexpr float F0_OV_MAX_HZ = 20000.f;

// What a call says about its overrides.  It travels from a pinned ring in front of the chunk and is read by the kernel, so none of it is baked into a plan or
// a captured graph.  mode 0: per-stream row buffers (cnt / rows of f0_override_kernel).  mode 1: the gather of a conversion -- the plan's stream s is window
// w0 + s of the recording (s < nw; the others are padding windows and keep the tracker's rows), row t of it is grid row (w0 + s) H - C + t.  With a list
// (the silence gate's compacted windows, silence.hip.h) the window is list[w0 + s] instead
struct F0OvCall { const float *grid; long long Nf; int mode, w0, nw, H, C, pad; const int *list; };

}  // namespace rvc
