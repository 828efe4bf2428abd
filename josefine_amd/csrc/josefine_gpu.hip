// josefine_gpu.hip — C ABI (include/josefine_gpu.h) of the MI355X batched
// Chained-Raft engine: host-side marshalling around the gfx950 kernels in
// jg_kernels.h.  There is deliberately no CPU implementation in this library:
// every entry point that computes does so on the device or fails with
// JG_EDEVICE.  What the host does do: validate arguments, bucket command rows by
// group (a stable radix sort of row indices — marshalling, not Raft), move bytes,
// and launch.
#include <cstring>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "jg_kernels.h"
#include "jg_route.h"
#include "jg_follower.h"
#include "jg_node.h"
#include "jg_load.h"
#include "jg_read.h"
#include "jg_move.h"
#include "jg_compact.h"
#include "jg_hosting.h"
#include "jg_watch.h"
#include "jg_isr.h"
#include "jg_isr_clock.h"
#include "jg_lookup.h"
#include "jg_commits.h"
#include "jg_await.h"
#include "jg_poll.h"

// The host side, by entry-point family (ONE translation unit: the pieces see each other's internals, in this order)
#include "jg_api_core.h"
#include "jg_api_drains.h"
#include "jg_api_engine.h"
#include "jg_api_node.h"
#include "jg_api_cluster.h"
#include "jg_api_routed.h"
#include "jg_api_misc.h"
#include "jg_api_manage.h"
#include "jg_api_load.h"
#include "jg_api_read.h"
#include "jg_api_move.h"
#include "jg_api_hosting.h"
#include "jg_api_lookup.h"
#include "jg_api_await.h"
#include "jg_api_poll.h"
#include "jg_api_feeds.h"
