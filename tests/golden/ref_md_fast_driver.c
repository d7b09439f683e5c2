/*
 * tests/golden/ref_md_fast_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the pieces of the reference's fast loop that can be called without the prediction tables ProductPerformFastLoop drags along, for
 * tests/golden/make_golden_md_fast.py and tests/test_md_fast_vs_ref.py.  Contains no reference code:
 *   drv_md_fast_sad      one entry of the reference's own NxMSadKernelSubSampled_funcPtrArray (Codec/EbComputeSAD.h:96-124), row asm_type
 *                        (0 ASM_NON_AVX2, 1 ASM_AVX2), column `index`: bwidth >> 3 for luma and bwidth >> 4 for chroma, as the caller
 *                        indexes it (Codec/EbProductCodingLoop.c:1337, :1352, :1364); returns -1 for an empty table entry
 *   drv_md_fast_rdcost   the RDCOST macro of Codec/EbRateDistortionCost.h:215-217, included where it lies
 *   drv_md_fast_pre_mode_decision   PreModeDecision (Codec/EbModeDecision.c:393-471) on n fabricated ModeDecisionCandidateBuffer_t whose
 *                        fast_cost_ptr and candidate_ptr->type are what the caller passes (type: 1 INTER_MODE, 2 INTRA_MODE, anything else
 *                        for a buffer no candidate was written into); best[] must hold 16 bytes
 * The buffer walk of ProductPerformFastLoop (:1284-1459) is NOT run here: it is restated in tests/md_fast_util.py.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "EbComputeSAD.h"
#include "EbModeDecision.h"
#include "EbRateDistortionCost.h"

/* the allocation bookkeeping EB_MALLOC writes to lives in EbEncHandle.c, which the link leaves out */
EbMemoryMapEntry *memoryMap;
uint32_t *memoryMapIndex;
uint64_t *totalLibMemory;
uint32_t libMallocCount, libThreadCount, libSemaphoreCount, libMutexCount;

int64_t drv_md_fast_sad(int asm_type, int index, const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride, uint32_t height,
                        uint32_t width)
{
    if (asm_type < 0 || asm_type >= ASM_TYPE_TOTAL || index < 0 || index > 16 || !NxMSadKernelSubSampled_funcPtrArray[asm_type][index]) return -1;
    return (int64_t)NxMSadKernelSubSampled_funcPtrArray[asm_type][index]((uint8_t *)src, src_stride, (uint8_t *)ref, ref_stride, height, width);
}

uint64_t drv_md_fast_rdcost(uint64_t lambda, uint64_t rate, uint64_t distortion) { return RDCOST(lambda, rate, distortion); }

int drv_md_fast_pre_mode_decision(int n, const uint64_t *cost, const uint8_t *type, uint32_t buffer_total_count, int same, uint8_t *best,
                                  uint32_t *full_count, uint8_t *disable_merge_index)
{
    if (n < 1 || n > 16) return -1;
    ModeDecisionCandidateBuffer_t *buffers = (ModeDecisionCandidateBuffer_t *)calloc((size_t)n, sizeof(*buffers));
    ModeDecisionCandidate_t *cands = (ModeDecisionCandidate_t *)calloc((size_t)n, sizeof(*cands));
    ModeDecisionCandidateBuffer_t *ptrs[16];
    uint64_t costs[16];
    for (int i = 0; i < n; i++) {
        costs[i] = cost[i];
        cands[i].type = type[i];
        buffers[i].fast_cost_ptr = &costs[i];
        buffers[i].candidate_ptr = &cands[i];
        ptrs[i] = &buffers[i];
    }
    *disable_merge_index = 0;   /* as the caller, :2552 */
    const EbErrorType rc = PreModeDecision(NULL, buffer_total_count, ptrs, full_count, best, disable_merge_index, same ? EB_TRUE : EB_FALSE);
    free(buffers);
    free(cands);
    return rc == EB_ErrorNone ? 0 : -2;
}
