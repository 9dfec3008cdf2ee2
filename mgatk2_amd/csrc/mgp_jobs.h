// mgp_jobs.h — the one way from the row jobs (mgp_jobs.hip: the txt and HDF5 writers, the
// variant and coverage passes, everything that reads a finished run's rows) into the engine's
// context (internal). mgp_jobs.hip sees mgp_ctx as an incomplete type.
#pragma once
#include "../../include/mgpileup.h"
#include "mgp_qc.h"

struct RowJobs;  // the jobs' buffers, kept for the next call (mgp_jobs.hip); a context owns one
RowJobs* row_jobs_new();
void row_jobs_free(RowJobs* jobs);  // (on the device its buffers were allocated on)

// What a job gets of a context whose run has finished
struct RunRows {
    int device;
    hipStream_t stream;
    int32_t n_cells;
    mgp::txtgz::Rows rows;
    mgp::qc::Tn5 tn5;
    RowJobs* jobs;
};
// mgp_engine.hip. The view of `ctx`'s last run: null check, mgp_sync, hipSetDevice, then
// MGP_E_STATE with "`no_run` (mgp_run first)" when the context has no run.
int run_rows(mgp_ctx* ctx, const char* no_run, RunRows* out);
// a context's device and jobs, no run needed (the *_fetch calls); ctx is not null
RowJobs* ctx_jobs(mgp_ctx* ctx, int* device);
