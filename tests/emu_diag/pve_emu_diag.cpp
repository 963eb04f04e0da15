// pve_emu_diag.cpp -- the CPU test emulator (tests/emu/pve_emu.cpp: the same C ABI, the same phase bodies) with the counters of
// PVE_EMU_DIAG (csrc/pve_tick_core.h) and a probe of RANK alone.  Test infrastructure of tests/test_rank_pairs_emulated.py.
#define PVE_EMU_DIAG 1
#include "../emu/pve_emu.cpp"

// lists of each length laid out / RANK fix-ups ([0] inside a pair, [1] others) since the last call
extern "C" void pve_emu_list_lengths(int *hist)
{
    for (int n = 0; n < 64; n++) { hist[n] = emu_diag_list_len[n]; emu_diag_list_len[n] = 0; }
}
extern "C" void pve_emu_rank_ties(int *ties)
{
    for (int n = 0; n < 2; n++) { ties[n] = emu_diag_ties[n]; emu_diag_ties[n] = 0; }
}

// RANK alone on hand-made lists: len[d] entries of list d, the first nown[d] its own-lane segment, vd / slot in pool order; the
// offsets, the pair table and the per-pair list bytes as LISTS / BUILD leave them.  stale: the sorted-index words start out
// carrying this tick's tag (left-over contents).  order[e]: the entry at sorted position e - loff[d] of e's list (-1 behind the
// list's finite entries); mypos[slot]: the position of the slot's own-lane entry (-1: it has none)
template <class ShT> static int emu_rank_probe(const int *len, const int *nown, const double *vd, const unsigned char *slot, int ticks, int stale,
                                               int *order, int *mypos)
{
    typedef Tick<128, ShT> T;
    ShT *shp = new ShT();
    ShT &sh = *shp;
    memset(&sh, 0, sizeof(sh));
    sh.hd.ticks = ticks;
    int e = 0, pairs = 0, own = 0;
    for (int d = 0; d < NL; d++) {
        e += len[d]; own += nown[d];
    }
    if (e > ShT::POOL || own > 128) { delete shp; return -1; }
    e = 0; own = 0;
    for (int d = 0; d < NL; d++) {
        sh.loff[d] = (int16_t)e; sh.lpo()[d] = e | (pairs << 16); sh.cstart[d] = (int16_t)own; sh.nfin[d] = 0;
        for (int q = 0; q < len[d]; q++) sh.u_list[pairs + q / 2] = (uint8_t)d;
        e += len[d]; pairs += (len[d] + 1) / 2; own += nown[d];
    }
    sh.loff[NL] = (int16_t)e; sh.lpo()[NL] = e | (pairs << 16); sh.cstart[NL] = (int16_t)own;
    for (int f = 0; f < e; f++) { sh.u_vd[f] = vd[f]; sh.u_slot[f] = slot[f]; order[f] = -1; }
    for (int d = 0; d < NL; d++) for (int f = sh.loff[d]; f < sh.loff[d + 1]; f++) sh.nfin[d] += vd[f] < INFINITY;
    if (stale) for (int f = 0; f < ShT::POOL; f++) sh.s_idx[f] = ((unsigned)ticks << 16) | (unsigned)(f % 7);
    for (int t = 0; t < 128; t++) T::template ph_rank<false>(t, sh);
    for (int d = 0; d < NL; d++) for (int q = 0; q < sh.nfin[d]; q++) order[sh.loff[d] + q] = sidx_at(sh.s_idx, sh.loff[d] + q) - sh.loff[d];
    for (int t = 0; t < 128; t++) mypos[t] = -1;
    for (int d = 0; d < NL; d++) for (int q = 0; q < nown[d]; q++) mypos[slot[sh.loff[d] + q]] = sh.mypos[slot[sh.loff[d] + q]];
    delete shp;
    return e;
}
extern "C" int pve_emu_rank_probe(int home, const int *len, const int *nown, const double *vd, const unsigned char *slot, int ticks, int stale,
                                  int *order, int *mypos)
{
    if (home) return emu_rank_probe<Shared<128, false, true>>(len, nown, vd, slot, ticks, stale, order, mypos);
    return emu_rank_probe<Shared<128>>(len, nown, vd, slot, ticks, stale, order, mypos);
}
