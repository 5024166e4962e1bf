// vgl_host.cpp -- host side of the C ABI declared in include/vcfgl_hip.h.
// Builds the constant tables a run needs (Poisson constants, beta shape parameters,
// fixed-qscore terms, qScore LUT, GL-model-1 error-model tables, rand48 jump tables),
// owns the device workspace, and enqueues the gfx950 kernels of vgl_sample.hip, vgl_serial.hip and vgl_gl.hip.
// There is no CPU compute path in this library.
//
// One translation unit (static linkage, hidden visibility and inlining span all of it), written as the units of hostlib/:
//   err.h          the last error text, HIPCHK, the environment hooks
//   mem.h          owners of device / pinned memory, streams and events
//   batch.h        the host batches (vgl_bgzf / stream / vcfin / inflate / bcfin _host_*) on those owners
//   tables.h       the constant tables, built on the host (pure)
//   plan.h         argument validation and the launch plan (pure)
//   ctx.h          the context: create, destroy, info, timing
//   tile_device.h  vgl_simulate_tile_device, the beta chain, vgl_dbg_*
//   outputs.h      text / BCF / gVCF / pileup / fetch-GL / set-alleles / discordance
//   slot.h         the host entry points: submit, deep reruns, vgl_tile_wait
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vcfgl_hip.h"
#include "vgl_device.h"
#include "vgl_inflate_core.h"
#include "vgl_bcfin_core.h"

#include "hostlib/err.h"
#include "hostlib/mem.h"
#include "hostlib/batch.h"
#include "hostlib/tables.h"
#include "hostlib/plan.h"
#include "hostlib/ctx.h"
#include "hostlib/tile_device.h"
#include "hostlib/outputs.h"
#include "hostlib/slot.h"
