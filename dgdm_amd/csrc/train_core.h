// What the three trainers (train2d.hip, train3d.hip, unet_train.hip) share and that is not GEMM-specific: the flat parameter banks with
// Adam and the by-name import / export, the elementwise kernels, the workspace arena.  Internal to the translation unit that includes
// it (anonymous namespace), as train_gemm.h.
#pragma once
#include "common.h"
#include <cmath>
#include <cstring>

namespace dgdm {
namespace {

// torch.optim.Adam (single-tensor form: lerp first moment, bias corrections on the host)
__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t n, float b1, float b2,
                            float eps, float wd, float step_size, float bc2_sqrt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gi = g[i];
    if (wd != 0.f) gi = fmaf(wd, p[i], gi);
    const float mi = m[i] + (gi - m[i]) * (1.f - b1);
    const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}
// dst (+)= src
__global__ void add_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = accumulate ? dst[i] + src[i] : src[i];
}
__global__ void scale_kernel(float *__restrict__ g, int64_t n, float f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] *= f;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Parameters, gradients and Adam's two moments as flat banks of n_params floats; a trainer derives from it and lays its tensors out
// with add_param.  `named` maps the reference's state_dict keys to offsets: bank 0 = the flat banks, bank 1 = a second bank that goes
// with the parameters only (BatchNorm running statistics).
struct ParamStore {
    struct Named { std::string name; size_t off; int64_t numel; int bank; };
    std::vector<Named> named;
    size_t n_params = 0;
    DevBuf P, G, M1, V, loss_dev;
    float beta1 = 0.9f, beta2 = 0.95f, eps = 1e-8f, wd = 0.f;
    int64_t adam_steps = 0;

    float *p(size_t o) const { return P.as<float>() + o; }
    float *gr(size_t o) const { return G.as<float>() + o; }
    size_t add_param(const std::string &name, int64_t numel) { named.push_back({name, n_params, numel, 0}); const size_t o = n_params; n_params += (size_t)numel; return o; }
    int alloc_banks() {
        int rc;
        for (DevBuf *b : {&P, &G, &M1, &V}) {
            if ((rc = b->alloc(n_params * sizeof(float)))) return rc;
            DGDM_HIP_CHECK(hipMemset(b->p, 0, n_params * sizeof(float)));
        }
        return loss_dev.alloc(64);
    }
    // one Adam step over the first n_trainable parameters; the trainer refreshes its derived weight copies afterwards
    int adam(float lr, size_t n_trainable, hipStream_t s) {
        ++adam_steps;
        const double bc1 = 1.0 - std::pow((double)beta1, (double)adam_steps), bc2 = 1.0 - std::pow((double)beta2, (double)adam_steps);
        hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n_trainable + 255) / 256)), dim3(256), 0, s, P.as<float>(), G.as<float>(), M1.as<float>(), V.as<float>(),
                           (int64_t)n_trainable, beta1, beta2, eps, wd, (float)((double)lr / bc1), (float)std::sqrt(bc2));
        DGDM_HIP_CHECK(hipGetLastError());
        return DGDM_OK;
    }
    // the first numel floats of a bank <-> a flat device vector (data-parallel exchange of gradients / running statistics)
    static int exchange(const DevBuf &bank, float *flat_dev, int64_t numel, int to_trainer, void *stream) {
        DGDM_HIP_CHECK(hipMemcpyAsync(to_trainer ? bank.p : (void *)flat_dev, to_trainer ? (const void *)flat_dev : bank.p, (size_t)numel * sizeof(float),
                                      hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return DGDM_OK;
    }
    int read_loss(float *loss_host, void *stream) const {
        if (!loss_host) return DGDM_OK;
        DGDM_HIP_CHECK(hipMemcpyAsync(loss_host, loss_dev.p, sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
        DGDM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        return DGDM_OK;
    }
    // by-name import (to_device) / export of `bank` (P, G, M1, V or a trainer's own bank of n_params floats) and, when given, of the
    // second bank `aux`; without `aux` the entries of bank 1 are skipped.  Synchronises; the caller refreshes what derives from P.
    int copy_state(DevBuf &bank, DevBuf *aux, const DgdmTensor *t, int n, bool to_device) {
        std::vector<float> host(n_params), host2(aux ? aux->bytes / sizeof(float) : 0);
        DGDM_HIP_CHECK(hipDeviceSynchronize());
        DGDM_HIP_CHECK(hipMemcpy(host.data(), bank.p, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        if (aux) DGDM_HIP_CHECK(hipMemcpy(host2.data(), aux->p, host2.size() * sizeof(float), hipMemcpyDeviceToHost));
        const StateDict sd(t, n);
        for (const Named &nm : named) {
            if (nm.bank != 0 && !aux) continue;
            float *user = const_cast<float *>(sd.f32(nm.name, nm.numel));
            if (!user) return DGDM_EKEY;
            float *mine = nm.bank == 0 ? &host[nm.off] : &host2[nm.off];
            if (to_device) memcpy(mine, user, (size_t)nm.numel * sizeof(float));
            else memcpy(user, mine, (size_t)nm.numel * sizeof(float));
        }
        if (to_device) {
            DGDM_HIP_CHECK(hipMemcpy(bank.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
            if (aux) DGDM_HIP_CHECK(hipMemcpy(aux->p, host2.data(), host2.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        return DGDM_OK;
    }
};

// A workspace carved out of one zero-filled allocation: every request is rounded up to 64 floats; one with a guard gets that many
// floats in front of and behind what its pointer addresses.
struct Arena {
    struct Want { void **ptr; int64_t n, guard; };
    std::vector<Want> want;
    template <class T> void add(T *&q, int64_t n, int64_t guard = 0) {
        static_assert(sizeof(T) == sizeof(float), "the arena counts in floats");
        want.push_back({(void **)&q, n, guard});
    }
    static int64_t span(const Want &w) { return (w.n + 2 * w.guard + 63) / 64 * 64; }
    int64_t floats() const { int64_t total = 0; for (const Want &w : want) total += span(w); return total; }
    int commit(DevBuf &ws) const {
        const size_t bytes = (size_t)floats() * sizeof(float);
        int rc = ws.alloc(bytes);
        if (rc) return rc;
        DGDM_HIP_CHECK(hipMemset(ws.p, 0, bytes));
        float *q = ws.as<float>();
        for (const Want &w : want) { *w.ptr = q + w.guard; q += span(w); }
        return DGDM_OK;
    }
};

}  // namespace
}  // namespace dgdm
