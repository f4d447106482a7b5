/* A stand-in for the collective library -- TEST INFRASTRUCTURE ONLY (tests/test_group_collectives.py).
 *
 * csrc/mm_group.hip exchanges the split-R-hat / ESS statistics through ncclAllGather / ncclAllReduce, and RCCL refuses two
 * ranks on one device, so on a one-GPU box that branch only ever ran with one rank.  This library exports the four entry
 * points the engine binds (mmcmc_group_bind_collectives) and carries them out with host threads and HIP copies, so N > 1
 * ranks can share one device: plain C against the HIP runtime API, no kernels, no assembly.
 *
 * The engine calls the collectives of one communicator from N host threads at once (one per shard).  A call publishes
 * its send pointer, meets the other ranks at a barrier, copies, and meets them again before anybody may publish the next
 * pointer.  Every barrier wait has a 30 s deadline; on expiry -- or when any rank has failed -- every rank's call returns
 * non-zero, which the engine turns into an error status: a rank that never arrives ends the test, it does not hang it.
 *
 * ncclAllReduce adds the ranks' buffers on the host in f32, in rank order from 0.0f: the order of the engine's host exchange
 * (acov[k] += a[k]), so the reduced lag sums are bit-identical to that branch's.
 *
 * FAKE_COLLECTIVES_FAIL_INIT in the environment makes ncclCommInitAll fail (the engine's exchange status -2). */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <errno.h>
#include <pthread.h>
#include <stddef.h>
#include <stdlib.h>
#include <time.h>

#define FAKE_FLOAT32 7 /* ncclFloat32 of the real header */
#define FAKE_SUM 0     /* ncclSum */
#define FAKE_DEADLINE_S 30

typedef struct fake_ctx {
    int n, refs;
    const void **send; /* [n]: what each rank published for the collective in flight */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int waiting;
    unsigned long generation;
    int failed;
} fake_ctx;

typedef struct fake_comm {
    fake_ctx *ctx;
    int rank;
} fake_comm;

static pthread_mutex_t g_count_mu = PTHREAD_MUTEX_INITIALIZER;
static size_t g_counts[4]; /* AllGather calls, AllReduce calls, last AllGather count, last AllReduce count */

static void count_call(int which, size_t count)
{
    pthread_mutex_lock(&g_count_mu);
    g_counts[which] += 1;
    g_counts[2 + which] = count;
    pthread_mutex_unlock(&g_count_mu);
}

void fake_collectives_counts(size_t out[4])
{
    pthread_mutex_lock(&g_count_mu);
    for (int i = 0; i < 4; ++i)
        out[i] = g_counts[i];
    pthread_mutex_unlock(&g_count_mu);
}

/* a rank that cannot go on tells the others, who then leave their barrier at once */
static int fail(fake_ctx *c)
{
    pthread_mutex_lock(&c->mu);
    c->failed = 1;
    pthread_cond_broadcast(&c->cv);
    pthread_mutex_unlock(&c->mu);
    return 1;
}

/* reusable barrier over the n ranks: 0 when all have arrived, non-zero on the deadline or a failed rank */
static int barrier(fake_ctx *c)
{
    struct timespec deadline;
    clock_gettime(CLOCK_REALTIME, &deadline);
    deadline.tv_sec += FAKE_DEADLINE_S;
    pthread_mutex_lock(&c->mu);
    if (c->failed) {
        pthread_mutex_unlock(&c->mu);
        return 1;
    }
    const unsigned long gen = c->generation;
    if (++c->waiting == c->n) {
        c->waiting = 0;
        c->generation += 1;
        pthread_cond_broadcast(&c->cv);
        pthread_mutex_unlock(&c->mu);
        return 0;
    }
    while (gen == c->generation && !c->failed)
        if (pthread_cond_timedwait(&c->cv, &c->mu, &deadline) == ETIMEDOUT && gen == c->generation) {
            c->failed = 1; /* the count of waiting ranks is stale from here on: the communicator stays failed */
            pthread_cond_broadcast(&c->cv);
        }
    const int released = gen != c->generation;
    pthread_mutex_unlock(&c->mu);
    return released ? 0 : 1;
}

int ncclCommInitAll(void **comms, int n, const int *devs)
{
    (void)devs; /* ranks may share a device: that is what this library is for */
    if (!comms || n < 1 || getenv("FAKE_COLLECTIVES_FAIL_INIT"))
        return 1;
    fake_ctx *c = (fake_ctx *)calloc(1, sizeof *c);
    if (!c)
        return 1;
    c->send = (const void **)calloc((size_t)n, sizeof *c->send);
    if (!c->send) {
        free(c);
        return 1;
    }
    c->n = n;
    pthread_mutex_init(&c->mu, NULL);
    pthread_cond_init(&c->cv, NULL);
    for (int r = 0; r < n; ++r) { /* one small comm per rank, each freed by its own ncclCommDestroy */
        fake_comm *k = (fake_comm *)malloc(sizeof *k);
        if (!k) {
            for (int q = 0; q < r; ++q)
                free(comms[q]);
            pthread_cond_destroy(&c->cv);
            pthread_mutex_destroy(&c->mu);
            free(c->send);
            free(c);
            return 1;
        }
        k->ctx = c;
        k->rank = r;
        comms[r] = k;
    }
    c->refs = n;
    return 0;
}

int ncclCommDestroy(void *comm)
{
    fake_comm *k = (fake_comm *)comm;
    if (!k)
        return 1;
    fake_ctx *c = k->ctx;
    pthread_mutex_lock(&c->mu);
    const int last = --c->refs == 0;
    pthread_mutex_unlock(&c->mu);
    free(k);
    if (last) {
        pthread_cond_destroy(&c->cv);
        pthread_mutex_destroy(&c->mu);
        free(c->send);
        free(c);
    }
    return 0;
}

int ncclAllGather(const void *send, void *recv, size_t count, int dtype, void *comm, hipStream_t stream)
{
    fake_comm *k = (fake_comm *)comm;
    if (dtype != FAKE_FLOAT32 || !k || !send || !recv)
        return 1;
    fake_ctx *c = k->ctx;
    count_call(0, count);
    c->send[k->rank] = send;
    if (barrier(c))
        return 1;
    for (int r = 0; r < c->n; ++r)
        if (hipMemcpyAsync((float *)recv + (size_t)r * count, c->send[r], count * sizeof(float), hipMemcpyDeviceToDevice, stream) !=
            hipSuccess)
            return fail(c);
    if (hipStreamSynchronize(stream) != hipSuccess)
        return fail(c);
    return barrier(c); /* nobody publishes the next pointer before every rank has read this one */
}

int ncclAllReduce(const void *send, void *recv, size_t count, int dtype, int op, void *comm, hipStream_t stream)
{
    fake_comm *k = (fake_comm *)comm;
    if (dtype != FAKE_FLOAT32 || op != FAKE_SUM || !k || !send || !recv)
        return 1;
    fake_ctx *c = k->ctx;
    count_call(1, count);
    c->send[k->rank] = send;
    if (barrier(c))
        return 1;
    float *part = (float *)malloc((count ? count : 1) * sizeof(float));
    float *sum = (float *)malloc((count ? count : 1) * sizeof(float));
    int bad = !part || !sum;
    for (size_t i = 0; !bad && i < count; ++i)
        sum[i] = 0.0f;
    for (int r = 0; !bad && r < c->n; ++r) {
        bad = hipMemcpyAsync(part, c->send[r], count * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess ||
              hipStreamSynchronize(stream) != hipSuccess;
        for (size_t i = 0; !bad && i < count; ++i)
            sum[i] += part[i];
    }
    if (!bad)
        bad = hipMemcpyAsync(recv, sum, count * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess ||
              hipStreamSynchronize(stream) != hipSuccess;
    free(part);
    free(sum);
    if (bad)
        return fail(c);
    return barrier(c);
}
