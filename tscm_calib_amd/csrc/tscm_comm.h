// tscm_comm.h -- what the LM driver may ask of a communicator (tscm_comm.hip: the RCCL, LOCAL and IPC exchange back-ends).
// tscm_comm stays opaque here: which back-end it is, whether it can still be used and how it becomes unusable are
// tscm_comm.hip's alone.  Host code only.  Every call that returns an int returns 0 or a TSCM_E_* code with its text in
// tscm_last_error().
#pragma once

#include "tscm/tscm.h"
#include "tscm_exec_plan.h"
#include "tscm_host.h"

#include <hip/hip_runtime.h>

#include <vector>

TSCM_INTERNAL tscm::CommKind comm_kind(const tscm_comm *c);        // kCommNone for NULL
TSCM_INTERNAL int comm_device(const tscm_comm *c);
TSCM_INTERNAL int comm_rank(const tscm_comm *c);
TSCM_INTERNAL int comm_world(const tscm_comm *c);
TSCM_INTERNAL bool comm_is_local_group(const tscm_comm *c);        // false for NULL
TSCM_INTERNAL bool comm_same_group(const tscm_comm *a, const tscm_comm *b);    // both of ONE tscm_comm_create_local call

// 0 while the communicator (may be NULL) can exchange: TSCM_E_RCCL once an RCCL one has been aborted, TSCM_E_PEER once an
// IPC one has lost a peer or a solve on it has failed
TSCM_INTERNAL int comm_usable(const tscm_comm *c);
// sum all-reduce of n doubles (in place) over the ranks of a multi-process communicator (RCCL, IPC), on `stream`
TSCM_INTERNAL int comm_allreduce(tscm_comm *c, double *buf, size_t n, hipStream_t stream);
// after a synchronisation: did an IPC exchange give up on a peer?  (TSCM_E_PEER, and the communicator is unusable)
TSCM_INTERNAL int comm_check(tscm_comm *c);
// waits for `stream`: a plain synchronisation without a communicator, with one rank or a local group; with a multi-rank RCCL
// communicator a poll under a watchdog that aborts the communicator (TSCM_E_RCCL) when the stream makes no progress
TSCM_INTERNAL int comm_wait(tscm_comm *c, hipStream_t stream);
// a solve on a multi-rank communicator has failed with something other than TSCM_E_INVALID: the ranks no longer agree on
// the exchanges made.  Aborts an RCCL communicator (the error text in place says so from then on), marks an IPC one dead
TSCM_INTERNAL void comm_fail(tscm_comm *c);

// LOCAL group: the one stream its members solve on; the members' exchange buffers for the solve that follows ([0, world) their
// T, [world, 2 world) their H_stage); the rank-order sum of n doubles over one of the two sets, on the group's stream
TSCM_INTERNAL hipStream_t comm_group_stream(const tscm_comm *c);
TSCM_INTERNAL int comm_group_bind(tscm_comm *c, const std::vector<double *> &ptrs);
TSCM_INTERNAL void comm_group_sum(tscm_comm *c, bool t_buffer, size_t n);
