// adam_step_body.h -- the body of the Adam step kernels of adam.hip, included INSIDE each of them (no include guard: a code
// fragment, not declarations), so that the kernel with the host's step_size keeps its instruction stream when a sibling with
// another source of step_size is added.  In scope where it is included: p, g, m, v, n, partial, nb, max_norm, gnorm_out, b1,
// b2, step_size, sqrt_bc2, eps, decay, pmax_bits, and `#pragma clang fp contract(off)` in force.
    __shared__ double sm[4];
    __shared__ float coef_s;
    double q = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) q += partial[i];
    q = block256_sum(q, sm);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(q);
        float coef = max_norm / (norm + 1e-6f);        // torch clip_grad_norm_
        coef = coef > 1.0f ? 1.0f : coef;
        if (!(max_norm > 0.f)) coef = 1.0f;            // max_norm <= 0: clipping disabled
        coef_s = coef;
        if (gnorm_out && blockIdx.x == 0) *gnorm_out = norm;
    }
    __syncthreads();
    const float coef = coef_s;
    float amax = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * coef;
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);          // exp_avg.lerp_(grad, 1-beta1)
        const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / sqrt_bc2 + eps;      // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
        const float pn = p[i] * decay - step_size * (mi / denom);
        p[i] = pn;
        amax = fmaxf(amax, pn == pn ? fabsf(pn) : __builtin_inff());      // a NaN parameter reads as "out of range"
    }
    if (pmax_bits) {       // max |param| after this step (bit patterns of non-negative floats order like the floats)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        __shared__ float wmax[4];
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = amax;
        __syncthreads();
        if (threadIdx.x == 0)      // ONE atomic per block: a few hundred to one address, not a few thousand
            atomicMax(pmax_bits, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
    }
