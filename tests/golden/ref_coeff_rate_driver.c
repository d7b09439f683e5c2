/* tests/golden/ref_coeff_rate_driver.c -- TEST INFRASTRUCTURE ONLY: drives the reference's own coefficient-rate code for the pins
 * of tests/test_coeff_rate_vs_ref.py and the fixture tests/golden/coeff_rate.npz (tests/golden/make_golden_rate.py links it against
 * the reference objects the oracle build compiled).  It contains no reference code, only calls into it:
 *   drv_init(base_qindex)  FRAME_CONTEXT from av1_default_coef_probs + init_mode_probs, then av1_estimate_syntax_rate and
 *                          av1_estimate_coefficients_rate into an MdRateEstimationContext_t, and setup_rtcd_internal(ASM_NON_AVX2)
 *                          (compiled here from aom_dsp_rtcd.h with RTCD_C, as the encoder's EbEncHandle.c does), which installs
 *                          av1_get_nz_map_contexts = av1_get_nz_map_contexts_sse2 (aom_dsp_rtcd.h:2211-2212);
 *   drv_tables(out)        the four fields of that context in the svthip_coeff_rate_tables layout (memcpy's, as a C host would);
 *   drv_bits(..)           Av1TuEstimateCoeffBits (Codec/EbRateDistortionCost.c:1350-1460) for one plane of one TU on caller-given
 *                          levels, through a minimal candidate buffer / candidate / coding unit / picture control set;
 *   drv_ext_tx_*           av1_ext_tx_used / get_ext_tx_set_type / allowed_tx_set_a / txsize_sqr_up_map for the candidate masks.
 * The layout of svthip_coeff_rate_tables is pinned against the reference's structs by the _Static_asserts below. */
#define RTCD_C
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "EbCabacContextModel.h"
#include "EbCodingUnit.h"
#include "EbEntropyCoding.h"
#include "EbMdRateEstimation.h"
#include "EbModeDecision.h"
#include "EbPictureControlSet.h"
#include "EbRateDistortionCost.h"

#include "../../include/svtav1_hip.h"

#define SAME_FIELD(a, b, f) \
    _Static_assert(sizeof(((a *)0)->f) == sizeof(((b *)0)->f) && offsetof(a, f) == offsetof(b, f), #f " differs from the reference")
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, txb_skip_cost);
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, base_eob_cost);
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, base_cost);
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, eob_extra_cost);
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, dc_sign_cost);
SAME_FIELD(LV_MAP_COEFF_COST, svthip_lv_map_coeff_cost, lps_cost);
_Static_assert(sizeof(LV_MAP_COEFF_COST) == sizeof(svthip_lv_map_coeff_cost), "LV_MAP_COEFF_COST size");
SAME_FIELD(LV_MAP_EOB_COST, svthip_lv_map_eob_cost, eob_cost);
_Static_assert(sizeof(LV_MAP_EOB_COST) == sizeof(svthip_lv_map_eob_cost), "LV_MAP_EOB_COST size");
#define SAME_SIZE(f) \
    _Static_assert(sizeof(((MdRateEstimationContext_t *)0)->f) == sizeof(((svthip_coeff_rate_tables *)0)->f), #f " size differs")
SAME_SIZE(coeffFacBits);
SAME_SIZE(eobFracBits);
SAME_SIZE(interTxTypeFacBits);
SAME_SIZE(intraTxTypeFacBits);

extern uint8_t allowed_tx_set_a[TX_SIZES_ALL][TX_TYPES];  // Codec/EbFullLoop.c:1095

static MdRateEstimationContext_t *g_md;

int drv_init(int base_qindex)
{
    FRAME_CONTEXT *fc = (FRAME_CONTEXT *)calloc(1, sizeof(FRAME_CONTEXT));
    if (!g_md) g_md = (MdRateEstimationContext_t *)calloc(1, sizeof(MdRateEstimationContext_t));
    if (!fc || !g_md) return -1;
    memset(g_md, 0, sizeof(*g_md));
    av1_default_coef_probs(fc, base_qindex);
    init_mode_probs(fc);
    av1_estimate_syntax_rate(g_md, EB_FALSE, fc);
    av1_estimate_coefficients_rate(g_md, fc);
    free(fc);
    setup_rtcd_internal(ASM_NON_AVX2);
    return 0;
}

void drv_tables(svthip_coeff_rate_tables *out)
{
    memcpy(out->coeffFacBits, g_md->coeffFacBits, sizeof(out->coeffFacBits));
    memcpy(out->eobFracBits, g_md->eobFracBits, sizeof(out->eobFracBits));
    memcpy(out->interTxTypeFacBits, g_md->interTxTypeFacBits, sizeof(out->interTxTypeFacBits));
    memcpy(out->intraTxTypeFacBits, g_md->intraTxTypeFacBits, sizeof(out->intraTxTypeFacBits));
}

/* levels: min(W,32) x min(H,32) int32, row stride min(W,32) (what Av1TuEstimateCoeffBits reads at tuOriginIndex 0) */
uint64_t drv_bits(const int32_t *levels, uint32_t eob, int plane_type, int tx_size, int tx_type, int txb_skip_ctx, int dc_sign_ctx, int is_inter,
                  int intra_mode, int reduced_tx_set)
{
    static ModeDecisionCandidate_t cand;
    static ModeDecisionCandidateBuffer_t buf;
    static CodingUnit_t cu;
    static PictureControlSet_t pcs;
    static PictureParentControlSet_t ppcs;
    static EbPictureBufferDesc_t coeffs;
    memset(&cand, 0, sizeof(cand));
    cand.type = is_inter ? INTER_MODE : INTRA_MODE;
    cand.pred_mode = (PredictionMode)intra_mode;
    cand.transform_type[PLANE_TYPE_Y] = cand.transform_type[PLANE_TYPE_UV] = (TxType)tx_type;
    cand.md_rate_estimation_ptr = g_md;
    buf.candidate_ptr = &cand;
    cu.luma_txb_skip_context = cu.cb_txb_skip_context = (int16_t)txb_skip_ctx;
    cu.luma_dc_sign_context = cu.cb_dc_sign_context = (int16_t)dc_sign_ctx;
    ppcs.reduced_tx_set_used = reduced_tx_set;
    pcs.parent_pcs_ptr = &ppcs;
    coeffs.bufferY = coeffs.bufferCb = coeffs.bufferCr = (EbByte)levels;
    uint64_t y = 0, cb = 0, cr = 0;
    Av1TuEstimateCoeffBits(&pcs, &buf, &cu, 0, 0, NULL, &coeffs, plane_type ? 0 : eob, plane_type ? eob : 0, 0, &y, &cb, &cr, (TxSize)tx_size,
                           (TxSize)tx_size, plane_type ? COMPONENT_CHROMA_CB : COMPONENT_LUMA, ASM_NON_AVX2);
    return plane_type ? cb : y;
}

int drv_ext_tx_set_type(int tx_size, int is_inter, int reduced) { return (int)get_ext_tx_set_type((TxSize)tx_size, is_inter, reduced); }
int drv_ext_tx_used(int set_type, int tx_type) { return av1_ext_tx_used[set_type][tx_type]; }
int drv_allowed_tx_set_a(int tx_size, int tx_type) { return allowed_tx_set_a[tx_size][tx_type]; }
int drv_txsize_sqr_up(int tx_size) { return (int)txsize_sqr_up_map[tx_size]; }
