// The load path of the plan cache as a program of its own, for a build of the HOST sources under sanitizers (make
// plan_load_check: -fsanitize=address,undefined).  For every file named on the command line: ehyb_plan_load, and where the file
// is accepted ehyb_plan_check, the column transcoder ehyb_plan_upload would run (ehyb_plan_device_cols), ehyb_plan_stats,
// ehyb_spmm_max_k, ehyb_plan_host_array of every array (every element read), ehyb_plan_destroy.  One line per file:
// "<path> accepted" or "<path> refused <code>".  Exit 0 unless a call on an accepted plan fails; a sanitizer report ends the
// program by itself.  No HIP runtime is linked: the few device-side symbols the host objects refer to are stubs here.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "ehyb_internal.h"

// (a loaded plan never reaches these: its panel streams are on the host, and nothing here uploads or multiplies)
int ehyb::materialize_panel_host(ehyb_plan*) { return EHYB_ERR_STATE; }
int ehyb::build_panel_on_device(ehyb_plan*) { return EHYB_ERR_STATE; }
extern "C" int ehyb_spmv_t_supported(const ehyb_plan*) { return EHYB_ERR_STATE; }  // (fsai.cpp asks; no FSAI is built here)
extern "C" void ehyb_plan_destroy(ehyb_plan* P) { delete P; }  // (nothing was uploaded: no device array to free)

namespace {

// every element of an array the plan hands out is read once
uint64_t touch(const void* p, int64_t count, size_t elem)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t sum = 0;
    for (size_t i = 0; i < (size_t)count * elem; ++i) sum += b[i];
    return sum;
}

const size_t kElem[] = {4, 4, 4, 4, 4, 4, 4, 8, 4, 4, 8, 4, 4, 8, 4, 4, 1, 4, 4, 4, 2, 8, 2, 4, 4, 2, 4, 4, 4, 4, 4, 2, 4, 4, 4, 4, 4};  // by EHYB_ARR_*
static_assert(sizeof kElem / sizeof kElem[0] == EHYB_ARR_PB_ITEMS1 + 1, "one element size per array of include/ehyb.h");

int walk(const char* path)
{
    ehyb_plan* plan = nullptr;
    int rc = ehyb_plan_load(path, 0, &plan, nullptr);
    if (rc != EHYB_OK) {
        printf("%s refused %d\n", path, rc);
        return plan == nullptr ? 0 : 1;  // a refused file leaves no plan behind
    }
    int bad = 0;
    uint64_t sum = 0;
    if ((rc = ehyb_plan_check(plan)) != EHYB_OK) bad = fprintf(stderr, "%s: loaded, then ehyb_plan_check: %d %s\n", path, rc, ehyb_last_error());
    const int64_t words = ehyb_plan_device_col_words(plan);
    ehyb_stats st;
    if ((rc = ehyb_plan_stats(plan, &st)) != EHYB_OK) bad = fprintf(stderr, "%s: ehyb_plan_stats: %d\n", path, rc);
    int k_max = 0;
    if ((rc = ehyb_spmm_max_k(plan, &k_max)) != EHYB_OK || k_max < 1) bad = fprintf(stderr, "%s: ehyb_spmm_max_k: %d, %d\n", path, rc, k_max);
    int64_t n_meta = 0;
    for (int which = 0; which <= EHYB_ARR_PB_ITEMS1; ++which) {
        const void* p = nullptr;
        int64_t count = 0;
        if ((rc = ehyb_plan_host_array(plan, which, &p, &count)) != EHYB_OK) {
            bad = fprintf(stderr, "%s: ehyb_plan_host_array(%d): %d %s\n", path, which, rc, ehyb_last_error());
            continue;
        }
        if (which == EHYB_ARR_SLAB_META) n_meta = count;
        if (p) sum += touch(p, count, kElem[which]);
    }
    if (words < 0) {
        bad = fprintf(stderr, "%s: ehyb_plan_device_col_words: %lld\n", path, (long long)words);
    } else {
        std::vector<uint32_t> w((size_t)words + 1), m((size_t)n_meta + 1);
        if ((rc = ehyb_plan_device_cols(plan, w.data(), m.data())) != EHYB_OK) bad = fprintf(stderr, "%s: ehyb_plan_device_cols: %d\n", path, rc);
        sum += touch(w.data(), words, 4) + touch(m.data(), n_meta, 4);
    }
    ehyb_plan_destroy(plan);
    printf("%s accepted %llx\n", path, (unsigned long long)sum);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv)
{
    int failed = 0;
    for (int i = 1; i < argc; ++i) failed |= walk(argv[i]);
    return failed;
}
