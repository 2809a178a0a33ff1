// comm.hip — RCCL on the context's stream (mm_comm_*, mm_allreduce_*, mm_allgather_*).
// Included from mastering.hip (its context helpers).

extern "C" {

int mm_comm_unique_id(char id_out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return MM_ERR_RCCL;
    static_assert(sizeof(id) == 128, "nccl unique id size");
    memcpy(id_out, &id, 128);
    return MM_OK;
}

int mm_comm_init(mm_ctx *c, int rank, int nranks, const char id[128]) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, nranks, uid, rank);
    if (r != ncclSuccess) return set_err(c, MM_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
    c->rank = rank;
    c->nranks = nranks;
    return MM_OK;
}

int mm_comm_destroy(mm_ctx *c) {
    if (!c) return MM_ERR_ARG;
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
    return MM_OK;
}

int mm_allreduce_sum_f64(mm_ctx *c, double *host_buf, int64_t n) {
    if (!c || !c->comm) return set_err(c, MM_ERR_STATE, "communicator not initialised");
    double *d;
    RET(get_buf(c, "coll", (size_t)std::max<int64_t>(n, 1), &d));
    HIPCHK(c, hipMemcpyAsync(d, host_buf, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = ncclAllReduce(d, d, (size_t)n, ncclDouble, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return set_err(c, MM_ERR_RCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
    HIPCHK(c, hipMemcpyAsync(host_buf, d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

// Device-pointer collectives on the context's stream: no host
// staging; the buffers must live on this context's device.  Synchronous on return.
int mm_allreduce_sum_f64_device(mm_ctx *c, double *d_buf, int64_t n) {
    if (!c) return MM_ERR_ARG;
    if (n < 0 || (n > 0 && !d_buf)) return set_err(c, MM_ERR_ARG, "all-reduce: bad buffer");
    if (!c->comm) return set_err(c, MM_ERR_STATE, "communicator not initialised");
    if (n > 0) {
        ncclResult_t r = ncclAllReduce(d_buf, d_buf, (size_t)n, ncclDouble, ncclSum, c->comm, c->stream);
        if (r != ncclSuccess) return set_err(c, MM_ERR_RCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

int mm_allgather_f64_device(mm_ctx *c, const double *d_in, double *d_out, int64_t n) {
    if (!c) return MM_ERR_ARG;
    if (n < 0 || (n > 0 && (!d_in || !d_out))) return set_err(c, MM_ERR_ARG, "all-gather: bad buffers");
    if (!c->comm) return set_err(c, MM_ERR_STATE, "communicator not initialised");
    if (n > 0) {
        ncclResult_t r = ncclAllGather(d_in, d_out, (size_t)n, ncclDouble, c->comm, c->stream);
        if (r != ncclSuccess) return set_err(c, MM_ERR_RCCL, "ncclAllGather: %s", ncclGetErrorString(r));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

int mm_allgather_f64(mm_ctx *c, const double *host_in, double *host_out, int64_t n) {
    if (!c || !c->comm) return set_err(c, MM_ERR_STATE, "communicator not initialised");
    double *d;
    RET(get_buf(c, "coll_ag", (size_t)std::max<int64_t>(n * (c->nranks + 1), 1), &d));
    double *dout = d + n;
    HIPCHK(c, hipMemcpyAsync(d, host_in, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = ncclAllGather(d, dout, (size_t)n, ncclDouble, c->comm, c->stream);
    if (r != ncclSuccess) return set_err(c, MM_ERR_RCCL, "ncclAllGather: %s", ncclGetErrorString(r));
    HIPCHK(c, hipMemcpyAsync(host_out, dout, n * c->nranks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

}  // extern "C"
