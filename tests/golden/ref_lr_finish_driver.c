/*
 * tests/golden/ref_lr_finish_driver.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Calls the reference's own restoration decision for tests/golden/make_golden_lr_finish.py.  Contains no reference code: it is
 * tests/golden/ref_lr_sgr_driver.c, which is tests/golden/ref_lr_driver.c (the reference's EbRestorationPick.c included where it lies at
 * build time, plus the picture scaffolding drv_lr_open / drv_lr_units / drv_lr_close) with the self-guided entry points (drv_sgr_filter is
 * the frame filter the chain pictures need), followed by entry points that only fill what rest_finish_search reads -- rusi_picture[plane]
 * of the picture, the three cost tables and rdmult of a Macroblock -- and call the reference's functions:
 *   drv_finish        rest_finish_search itself for the frame and unit types; then, for the numbers it keeps to itself, its own per-plane
 *                     sequence of search_rest_type_finish calls on one scratch zeroed once (as rest_finish_search allocates it), noting
 *                     rsc.sse, rsc.bits, the returned cost and best_rtype after the walks.  The frame types of the two are compared.
 *   drv_finish_bits   count_wiener_bits / count_sgrproj_bits alone
 *   drv_finish_time   seconds of rest_finish_search, repeated (the CPU yardstick of tools/lr_finish_probe.py)
 * A picture must be open (drv_lr_open): its size and unit sizes give the unit counts; no sample is read.
 */
#include "ref_lr_sgr_driver.c"

static Macroblock FX;

static void finish_fill(const int32_t rates[8], const int32_t unit_base[4], const int64_t *wiener_sse, const int16_t *taps, const int64_t *sgr_sse,
                        const int32_t *sgrproj)
{
    memset(&FX, 0, sizeof(FX));
    FX.rdmult = rates[0];
    FX.wiener_restore_cost[0] = rates[1], FX.wiener_restore_cost[1] = rates[2];
    FX.sgrproj_restore_cost[0] = rates[3], FX.sgrproj_restore_cost[1] = rates[4];
    for (int i = 0; i < 3; i++) FX.switchable_restore_cost[i] = rates[5 + i];
    for (int p = 0; p < 3; p++) {
        const int n = G.cm.rst_info[p].units_per_tile;
        RestUnitSearchInfo *r = (RestUnitSearchInfo *)calloc(n, sizeof(*r));
        G.ppcs->rusi_picture[p] = r;
        for (int i = 0; i < n; i++) {
            const int u = unit_base[p] + i;
            r[i].sse[RESTORE_NONE] = wiener_sse[2 * u], r[i].sse[RESTORE_WIENER] = wiener_sse[2 * u + 1], r[i].sse[RESTORE_SGRPROJ] = sgr_sse[u];
            memcpy(r[i].wiener.vfilter, taps + 16 * u, 16);
            memcpy(r[i].wiener.hfilter, taps + 16 * u + 8, 16);
            r[i].sgrproj.ep = sgrproj[4 * u], r[i].sgrproj.xqd[0] = sgrproj[4 * u + 1], r[i].sgrproj.xqd[1] = sgrproj[4 * u + 2];
        }
    }
}

static void finish_free(void)
{
    for (int p = 0; p < 3; p++) free(G.ppcs->rusi_picture[p]), G.ppcs->rusi_picture[p] = NULL;
}

/* rates[8] = rdmult, wiener[2], sgrproj[2], switchable[3]; the tables by unit_base[p] + the unit's index.  Outputs: unit_type[units],
 * frame_type[3], best_rtype[units][4] (WIENER, SGRPROJ, SWITCHABLE walk -- 0 where not tried -- then 0), sse / bits / cost [3][4],
 * n_tried[3].  Returns the number of planes whose frame type differs between rest_finish_search and the walks called one by one. */
int drv_finish(const int32_t rates[8], const int32_t unit_base[4], const int64_t *wiener_sse, const int16_t *taps, const int64_t *sgr_sse,
               const int32_t *sgrproj, uint8_t *unit_type, int32_t *frame_type, uint8_t *best_rtype, int64_t *sse, int64_t *bits, double *cost,
               int32_t *n_tried)
{
    int differ = 0;
    finish_fill(rates, unit_base, wiener_sse, taps, sgr_sse, sgrproj);
    for (int p = 0; p < 3; p++) memset(G.cm.rst_info[p].unit_info, 0, sizeof(RestorationUnitInfo) * G.cm.rst_info[p].units_per_tile);
    rest_finish_search(&FX, &G.cm);
    for (int p = 0; p < 3; p++) {
        const RestorationInfo *rsi = &G.cm.rst_info[p];
        frame_type[p] = rsi->frame_restoration_type;
        for (int i = 0; i < rsi->units_per_tile; i++)
            unit_type[unit_base[p] + i] = rsi->frame_restoration_type == RESTORE_NONE ? RESTORE_NONE : rsi->unit_info[i].restoration_type;
    }
    /* the walks one by one */
    RestUnitSearchInfo *scratch = (RestUnitSearchInfo *)calloc(G.cm.rst_info[0].units_per_tile, sizeof(*scratch));
    for (int p = 0; p < 3; p++) {
        const int n = G.cm.rst_info[p].units_per_tile, tried = n > 1 ? RESTORE_TYPES : RESTORE_SWITCHABLE_TYPES;
        RestSearchCtxt rsc;
        memset(&rsc, 0, sizeof(rsc));
        rsc.cm = &G.cm, rsc.x = &FX, rsc.plane = p, rsc.rusi = scratch, rsc.rusi_pic = G.ppcs->rusi_picture[p];
        int best = 0;
        double best_cost = 0;
        for (int r = 0; r < 4; r++) sse[4 * p + r] = bits[4 * p + r] = 0, cost[4 * p + r] = 0;
        for (int r = 0; r < tried; r++) {
            const double c = search_rest_type_finish(&rsc, (RestorationType)r);
            sse[4 * p + r] = rsc.sse, bits[4 * p + r] = rsc.bits, cost[4 * p + r] = c;
            if (r == 0 || c < best_cost) best_cost = c, best = r;
        }
        n_tried[p] = tried;
        differ += best != frame_type[p];
        for (int i = 0; i < n; i++) {
            uint8_t *b = best_rtype + 4 * (unit_base[p] + i);
            b[0] = scratch[i].best_rtype[0], b[1] = scratch[i].best_rtype[1], b[2] = tried == RESTORE_TYPES ? scratch[i].best_rtype[2] : 0, b[3] = 0;
        }
    }
    free(scratch);
    finish_free();
    return differ;
}

/* n jobs: win[n] (7 or 5), taps[n][6] and ref[n][6] = vfilter 0-2, hfilter 0-2 -> wiener_bits[n]; sgr[n][3] = ep, xqd0, xqd1 and
 * sgr_ref[n][2] -> sgr_bits[n] */
void drv_finish_bits(int n, const int32_t *win, const int32_t *taps, const int32_t *ref, const int32_t *sgr, const int32_t *sgr_ref, int32_t *wiener_bits,
                     int32_t *sgr_bits)
{
    for (int i = 0; i < n; i++) {
        WienerInfo a, b;
        SgrprojInfo s, t;
        memset(&a, 0, sizeof(a)), memset(&b, 0, sizeof(b));
        for (int j = 0; j < 3; j++) {
            a.vfilter[j] = taps[6 * i + j], a.hfilter[j] = taps[6 * i + 3 + j];
            b.vfilter[j] = ref[6 * i + j], b.hfilter[j] = ref[6 * i + 3 + j];
        }
        wiener_bits[i] = count_wiener_bits(win[i], &a, &b);
        s.ep = sgr[3 * i], s.xqd[0] = sgr[3 * i + 1], s.xqd[1] = sgr[3 * i + 2];
        t.ep = 0, t.xqd[0] = sgr_ref[2 * i], t.xqd[1] = sgr_ref[2 * i + 1];
        sgr_bits[i] = count_sgrproj_bits(&s, &t);
    }
}

/* seconds of `repeat` calls of rest_finish_search on the tables given */
double drv_finish_time(const int32_t rates[8], const int32_t unit_base[4], const int64_t *wiener_sse, const int16_t *taps, const int64_t *sgr_sse,
                       const int32_t *sgrproj, int repeat)
{
    struct timespec a, b;
    finish_fill(rates, unit_base, wiener_sse, taps, sgr_sse, sgrproj);
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < repeat; i++) rest_finish_search(&FX, &G.cm);
    clock_gettime(CLOCK_MONOTONIC, &b);
    finish_free();
    return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
}
