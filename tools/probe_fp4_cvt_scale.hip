// Does v_cvt_scalef32_pk_{f16,bf16,f32}_fp4 honour the MANTISSA of its f32 scale operand, or only its exponent?  (the NVFP4
// fold of csrc/nvfp4_linear.hip is built so that it does not depend on the answer.)  All 16 e2m1 codes x all 127 e4m3 scale codes
// 0x00 .. 0x7E, the scale handed over as its exact f32 value; every result is compared bit for bit with the exact product and with the
// product by the scale's power of two alone.  Prints one JSON line.
//     hipcc --offload-arch=gfx950 -O2 tools/probe_fp4_cvt_scale.hip -o build_variant/probe_fp4_cvt_scale && build_variant/probe_fp4_cvt_scale
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

__global__ void probe_kernel(const float* scale, float* out) {          // out[(s * 16 + c) * 3 + {f16, bf16, f32}], all widened to f32
    const int s = blockIdx.x, c = threadIdx.x;
    const uint32_t w = (uint32_t)c;                                      // the code in the low nibble of byte 0
    const float sf = scale[s];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const h2 h = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sf, 0);
    const b2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sf, 0);
    const f2 f = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 0);
    out[(s * 16 + c) * 3 + 0] = (float)h.x;
    out[(s * 16 + c) * 3 + 1] = (float)b.x;
    out[(s * 16 + c) * 3 + 2] = f.x;
}

int main() {
    static const double mag[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
    float scale[127], pow2[127];
    for (int s = 0; s < 127; ++s) {
        const int e = s >> 3, m = s & 7;
        scale[s] = e ? (float)std::ldexp(1.0 + m / 8.0, e - 7) : (float)std::ldexp(m / 8.0, -6);
        int ex = 0;
        pow2[s] = scale[s] == 0.f ? 0.f : (float)std::ldexp(1.0, (std::frexp(scale[s], &ex), ex - 1));
    }
    float *d_scale = nullptr, *d_out = nullptr;
    static float out[127 * 16 * 3];
    if (hipMalloc((void**)&d_scale, sizeof(scale)) || hipMalloc((void**)&d_out, sizeof(out))) return 2;
    if (hipMemcpy(d_scale, scale, sizeof(scale), hipMemcpyHostToDevice)) return 2;
    hipLaunchKernelGGL(probe_kernel, dim3(127), dim3(16), 0, 0, d_scale, d_out);
    if (hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost)) return 2;
    static const char* names[3] = {"f16", "bf16", "f32"};
    std::printf("{\"probe\": \"cvt_scalef32_pk_fp4\"");
    for (int t = 0; t < 3; ++t) {
        int exact = 0, exp_only = 0, other = 0, total = 0;
        for (int s = 8; s < 127; ++s)                                    // normal scales with a non-zero mantissa tell the two apart
            for (int c = 0; c < 16; ++c) {
                if ((s & 7) == 0 || (c & 7) == 0) continue;
                const float got = out[(s * 16 + c) * 3 + t];
                const double sign = c & 8 ? -1.0 : 1.0;
                const float full = (float)(sign * mag[c & 7] * scale[s]), trunc = (float)(sign * mag[c & 7] * pow2[s]);
                ++total;
                if (std::memcmp(&got, &full, 4) == 0) ++exact;
                else if (std::memcmp(&got, &trunc, 4) == 0) ++exp_only;
                else ++other;
            }
        std::printf(", \"%s\": {\"cases\": %d, \"exact_product\": %d, \"exponent_only\": %d, \"other\": %d}", names[t], total, exact, exp_only, other);
    }
    std::printf("}\n");
    (void)hipFree(d_scale);
    (void)hipFree(d_out);
    return 0;
}
