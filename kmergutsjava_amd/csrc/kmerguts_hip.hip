// kmerguts_hip.hip -- host side of libkmerguts_hip.so (C ABI in include/kmerguts_hip.h).
//
// Replaces, for a batch of sequences, the reference's run() body between readFasta and the
// report printers (KGJ:776-816): prepareQuery/addKmers, the query sort, lookup and
// gatherHits/processSetOfHits.  Everything runs on one HIP stream owned by the table object;
// scratch and results come from a per-table cache of device blocks (DevCache) so that repeated
// scans reuse the same HBM.
//
// This file is the table of contents of the one translation unit: the kernel headers, then the host files in dependency order.
#include "kg_device.hpp"
#include "kg_aggregate.hpp"
#include "kg_partition.hpp"
#include "kg_order.hpp"
#include "kg_build.hpp"
#include "kg_merge.hpp"
#include "kg_derive.hpp"
#include "kg_cluster.hpp"
#include "kg_align.hpp"
#include "kg_band.hpp"
#include "kg_trace.hpp"
#include "kg_ops.hpp"
#include "kg_search.hpp"
#include "kg_ungapped.hpp"
#include "kg_seed.hpp"
#include "kg_searchdb.hpp"
#include "kg_mask.hpp"
#include "kg_assign.hpp"
#include "kg_regions.hpp"
#include "kg_orfs.hpp"
#include "kg_coding.hpp"
#include "kg_starts.hpp"
#include "kg_repair.hpp"
#include "kg_select.hpp"
#include "kg_votes.hpp"
#include "kg_compose.hpp"
#include "kg_evidence.hpp"
#include "kg_residual.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <cerrno>
#include <cmath>

// ---- what every host file needs, then the table, the result and the scan ----
#include "kg_host.hpp"
#include "kg_host_table.hpp"
#include "kg_host_result.hpp"
#include "kg_host_plan.hpp"
#include "kg_host_aggregate.hpp"
#include "kg_host_scan.hpp"

// ---- the batch stages: each host beside its kernels ----
#include "kg_host_build.hpp"
#include "kg_host_derive.hpp"
#include "kg_host_merge.hpp"
#include "kg_host_align.hpp"
#include "kg_host_trace.hpp"
#include "kg_host_mask.hpp"
#include "kg_host_cluster.hpp"
#include "kg_host_search.hpp"
#include "kg_host_searchdb.hpp"
#include "kg_host_assign.hpp"
#include "kg_host_regions.hpp"
#include "kg_host_orfs.hpp"
#include "kg_host_repair.hpp"
#include "kg_host_coding.hpp"
#include "kg_host_starts.hpp"
#include "kg_host_select.hpp"
#include "kg_host_votes.hpp"
#include "kg_host_compose.hpp"
#include "kg_host_evidence.hpp"
#include "kg_host_residual.hpp"
