// bsa_snv.cpp -- SNV calling over the columns of a window's MSA (include/bsalign_msa.h: bsa_msa_call_snvs, bsa_msa_snv_text), and the tables the
// device form (bsa_window_snv.hip) takes from here so that host and device share one libm.
//
// The definition is the reference's (call_snvs_bspoa, bspoa.h:4931-5049, printed by print_snvs_bspoa :5053-5089): per column the two most frequent
// of A C G T among the voting rows; a window-wide estimate of the error rate from a histogram of (second allele count, coverage) -- each entry
// spreads a binomial likelihood over a grid of 100 rates, the grid value with the largest sum above 1 wins, else 0.01 --; a column is a call if the
// second allele is frequent enough, the two cover enough rows and the binomial tail of seeing the second allele that often by error is small enough.
//
// Organisation here (not the reference's): what an (altn, covn) entry adds to the grid is a ROW of weights that depends on nothing else, so it is
// formed once (snv_row) -- by the host form for every entry it meets, by the device model for every entry a window can hold -- and the sums are
// float multiply, float add, in ascending entry order, as there.  This file is built without contraction to multiply-add.
#include "../../include/bsalign_msa.h"
#include "../../include/bsalign_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr uint32_t kGrid = 100;                // rates on the grid
constexpr float kStep = 0.0005f;               // their distance
constexpr float kMinProb = 0.01f;              // a direction of the spread stops behind the first weight at or below this
constexpr float kDefaultRate = 0.01f;          // the estimate where no grid value gathers more than 1
constexpr uint32_t kMaxRows = 1000;            // the log-factorial table ends here (bspoa.h:3390)
constexpr uint32_t kMaxCols = 65535;           // the histogram's counters are 16 bits there

struct LogFactorial {
	double v[kMaxRows + 1];
	LogFactorial(){ v[0] = 0; for(uint32_t k = 1; k <= kMaxRows; k++) v[k] = v[k - 1] + std::log((double)k); }
};

// log of the binomial probability of m events in n trials at rate p (cal_binomial_bspoa, bspoa.h:3404)
inline double binomial_log(const LogFactorial &lf, uint32_t n, uint32_t m, double p){
	return std::log(p) * m + std::log(1 - p) * (n - m) + (lf.v[n] - lf.v[m] - lf.v[n - m]);
}

// What one (altn, covn) entry adds to the grid: w[first .. first + n) for a count of one.  Returns false where the entry's own rate falls off the grid.
bool snv_row(const LogFactorial &lf, uint32_t altn, uint32_t covn, uint32_t *first, uint32_t *n, float *w /* kGrid */){
	const float pexp = (float)(1.0 * altn / covn);
	const int j = (int)(pexp / kStep);
	if(!(j > 0 && j < (int)kGrid)) return false;
	uint32_t lo = (uint32_t)j, hi = (uint32_t)j;
	for(uint32_t k = 0; k < (uint32_t)j; k++){
		const float perr = pexp - kStep * k;
		const float prob = (float)std::exp(binomial_log(lf, covn, altn, perr));
		w[lo = j - k] = prob;
		if(prob <= kMinProb) break;
	}
	for(uint32_t k = 1; j + k < kGrid; k++){
		const float perr = pexp + kStep * k;
		const float prob = (float)std::exp(binomial_log(lf, covn, altn, perr));
		w[hi = j + k] = prob;
		if(prob <= kMinProb) break;
	}
	*first = lo; *n = hi - lo + 1;
	return true;
}

struct Top2 { uint32_t cnt[5], covn, m1, m2; };
inline Top2 top2(const uint8_t *col, uint32_t r0, uint32_t nseq){
	Top2 t = { {0, 0, 0, 0, 0}, 0, 0, 1 };
	for(uint32_t r = r0; r < nseq; r++) if(col[r] <= 4){ t.cnt[col[r]]++; t.covn++; }
	if(t.cnt[0] < t.cnt[1]){ t.m1 = 1; t.m2 = 0; }
	for(uint32_t i = 2; i < 4; i++){
		if(t.cnt[i] > t.cnt[t.m1]){ t.m2 = t.m1; t.m1 = i; }
		else if(t.cnt[i] > t.cnt[t.m2]) t.m2 = i;
	}
	return t;
}

inline uint32_t min_cover(uint32_t realnseq, float min_covfrq){
	const float f = (float)realnseq * min_covfrq;
	return (uint32_t)(uint16_t)(2 > f ? 2.0f : f);
}

inline bool params_ok(const bsa_snv_params_t *par){
	return par && par->skip_first_row <= 1u && par->min_covfrq >= 0.0f && par->min_covfrq <= 65.0f;       // (1000 rows x 65 still fits the 16 bits of mincov)
}

inline const uint8_t *column(const uint8_t *cols, const uint32_t *idxs, size_t mrow, uint32_t i){
	return cols + (size_t)(idxs ? idxs[i] : i) * mrow;
}

struct Sink {
	char *out; size_t cap, n;
	void put(const char *p, size_t len){
		if(out && n + len <= cap) memcpy(out + n, p, len);
		n += len;
	}
};

}  // namespace

extern "C" int bsa_snv_params_check_internal(const bsa_snv_params_t *par){ return params_ok(par) ? BSA_OK : BSA_E_ARG; }

extern "C" int bsa_msa_call_snvs(const uint8_t *cols, const uint32_t *idxs, uint32_t nall, uint32_t nseq, uint32_t mlen, const bsa_snv_params_t *par,
		bsa_snv_t *snv, size_t snv_cap, size_t *nsnv, float *pexp_out, uint32_t *nsites_out){
	if(!params_ok(par) || !nsnv || (mlen && !cols) || nseq > nall || nall < 1u || (snv_cap && !snv)) return BSA_E_ARG;
	*nsnv = 0;
	if(pexp_out) *pexp_out = kDefaultRate;
	if(nsites_out) *nsites_out = 0;
	if(nseq > kMaxRows || mlen > kMaxCols) return BSA_E_UNSUPPORTED;
	static const LogFactorial lf;
	const size_t mrow = (size_t)nall + 3;
	const uint32_t r0 = par->skip_first_row, realnseq = nseq > r0 ? nseq - r0 : 0u;
	const uint32_t mincov = min_cover(realnseq, par->min_covfrq);

	// the histogram: acnts[altn * realnseq + covn - 1], altn <= covn / 2
	std::vector<uint16_t> acnts((size_t)realnseq * (realnseq / 2 + 1) + 1, 0);
	uint32_t nsites = 0;
	for(uint32_t pos = 0; pos < mlen; pos++){
		const Top2 t = top2(column(cols, idxs, mrow, pos), r0, nseq);
		if(t.cnt[t.m1] + t.cnt[t.m2] >= mincov){ acnts[(size_t)t.cnt[t.m2] * realnseq + t.covn - 1]++; nsites++; }
	}
	float psums[kGrid], w[kGrid];
	for(uint32_t i = 0; i < kGrid; i++) psums[i] = 0;
	for(size_t i = 1; i + 1 < acnts.size(); i++){
		if(acnts[i] == 0) continue;
		uint32_t first, n;
		if(!snv_row(lf, (uint32_t)(i / realnseq), (uint32_t)(i % realnseq) + 1, &first, &n, w)) continue;
		for(uint32_t b = first; b < first + n; b++) psums[b] += acnts[i] * w[b];
	}
	float best = 1, pexp = kDefaultRate;
	for(uint32_t i = 0; i < kGrid; i++) if(best < psums[i]){ pexp = i * kStep; best = psums[i]; }
	if(pexp_out) *pexp_out = pexp;
	if(nsites_out) *nsites_out = nsites;

	const double ln10 = std::log(10.0);
	size_t n = 0;
	uint32_t cpos = 0, lpos = 0;
	for(uint32_t pos = 0; pos < mlen; pos++){
		const uint8_t *col = column(cols, idxs, mrow, pos);
		const Top2 t = top2(col, r0, nseq);
		const uint32_t refn = t.cnt[t.m1], altn = t.cnt[t.m2];
		if((int64_t)altn >= (int64_t)par->min_varcnt && refn + altn >= mincov){
			const float lp = (float)binomial_log(lf, t.covn, altn, pexp);
			const double q = -(lp / ln10);
			uint32_t qual = q >= 1000.0 ? 1000u : q > 0.0 ? (uint32_t)q : 0u;
			if(qual >= par->min_snvqlt){
				if(n < snv_cap){
					bsa_snv_t v;
					memset(&v, 0, sizeof(v));
					v.mpos = pos; v.cpos = cpos; v.lpos = lpos; v.qual = qual;
					v.covn = (uint16_t)t.covn; v.refn = (uint16_t)refn; v.altn = (uint16_t)altn; v.refb = (uint8_t)t.m1; v.altb = (uint8_t)t.m2;
					snv[n] = v;
				}
				n++;
			}
		}
		if(col[nall] < 4) cpos++;
		if(col[nall - 1] < 4) lpos++;
	}
	*nsnv = n;
	return n <= snv_cap ? BSA_OK : BSA_E_NOMEM;
}

// print_snvs_bspoa: one line a record -- label, cpos, mpos, the five consensus bases in front with their qualities, reference and alternative base
// with their counts, the five behind, coverage, quality, and the column's rows as a genotype string
extern "C" int bsa_msa_snv_text(const uint8_t *cols, const uint32_t *idxs, uint32_t nall, uint32_t nseq, uint32_t mlen, const uint8_t *cns, const uint8_t *qlt, uint32_t clen,
		const bsa_snv_t *snv, size_t nsnv, const char *label, char *out, size_t cap, size_t *need){
	if(!need || !label || (nsnv && (!snv || !cols)) || (clen && (!cns || !qlt)) || nseq > nall) return BSA_E_ARG;
	static const char base[] = "ACGTN-acgtn*", geno[] = "ACGT-.*";
	const size_t mrow = (size_t)nall + 3;
	Sink s{out, cap, 0};
	std::string line;
	for(size_t k = 0; k < nsnv; k++){
		const bsa_snv_t &v = snv[k];
		if(v.mpos >= mlen || v.cpos >= clen || v.refb > 3 || v.altb > 3) return BSA_E_ARG;
		char fl[4][6], num[64];
		uint32_t f = v.cpos < 5u ? v.cpos : 5u;
		for(uint32_t j = 0; j < f; j++){ fl[0][j] = base[cns[v.cpos - f + j] % 12u]; fl[2][j] = (char)(qlt[v.cpos - f + j] + '!'); }
		fl[0][f] = fl[2][f] = 0;
		f = clen - v.cpos - 1u < 5u ? clen - v.cpos - 1u : 5u;
		for(uint32_t j = 0; j < f; j++){ fl[1][j] = base[cns[v.cpos + 1 + j] % 12u]; fl[3][j] = (char)(qlt[v.cpos + 1 + j] + '!'); }
		fl[1][f] = fl[3][f] = 0;
		line.assign(label); line += " SNP\t";
		snprintf(num, sizeof(num), "%d\t%d\t", (int)v.cpos, (int)v.mpos); line += num;
		line += fl[0]; line += '\t'; line += fl[2]; line += '\t';
		snprintf(num, sizeof(num), "%c\t%d\t%c\t%d\t", base[v.refb], (int)v.refn, base[v.altb], (int)v.altn); line += num;
		line += fl[1]; line += '\t'; line += fl[3]; line += '\t';
		snprintf(num, sizeof(num), "%d\t%d\t", (int)v.covn, (int)v.qual); line += num;
		const uint8_t *col = column(cols, idxs, mrow, v.mpos);
		for(uint32_t r = 0; r < nseq; r++) line += geno[col[r] < 7 ? col[r] : 5];
		line += '\n';
		s.put(line.data(), line.size());
	}
	*need = s.n;
	return (out && s.n <= cap) ? BSA_OK : BSA_E_NOMEM;
}

// The device model's tables, by the code above: lf[k] = log(k!), k <= 1000;  lgp[i] / lg1p[i] = log(p) / log(1 - p) of the grid value i * 0.0005f
// (i < 100; entry 0 is never an estimate and holds 0) and of the default 0.01f (i == 100), pgrid[i] the values themselves;  the rows of every
// (altn, covn), covn <= max_rows, whose own rate lies on the grid, in ascending (altn, covn): for altn = 1 .. *amax the admitted covn are
// cmin[altn] .. max_rows (row rowbase[altn] + covn - cmin[altn]; rowbase[*amax + 1] = the number of rows), desc[2 r] = where row r's weights begin,
// desc[2 r + 1] = first bin | bins << 8.  desc / weights NULL: the numbers only.  BSA_E_UNSUPPORTED where the admitted covn of an altn are not one
// range that ends at max_rows, or the ranges do not shrink with altn (the arithmetic is monotone: it does not happen).
extern "C" int bsa_snv_model_internal(uint32_t max_rows, double *lfv, double *lgp, double *lg1p, float *pgrid, double *ln10, uint32_t *amax, uint32_t *cmin, uint32_t *rowbase,
		uint32_t *desc, float *weights, size_t *nrows, size_t *nweights){
	if(max_rows > kMaxRows) return BSA_E_UNSUPPORTED;
	static const LogFactorial lf;
	if(lfv) memcpy(lfv, lf.v, sizeof(lf.v));
	for(uint32_t i = 0; i <= kGrid; i++){
		const float p = i < kGrid ? i * kStep : kDefaultRate;
		if(pgrid) pgrid[i] = p;
		if(lgp) lgp[i] = i ? std::log((double)p) : 0.0;
		if(lg1p) lg1p[i] = i ? std::log(1 - (double)p) : 0.0;
	}
	if(ln10) *ln10 = std::log(10.0);
	size_t nr = 0, nw = 0;
	uint32_t a = 1, prev_cmin = 0;
	float w[kGrid];
	for(; a <= max_rows; a++){
		uint32_t c0 = 0, first, n;
		for(uint32_t c = a; c <= max_rows; c++){
			const bool ok = snv_row(lf, a, c, &first, &n, w);
			if(ok && !c0) c0 = c;
			if(!ok && c0) return BSA_E_UNSUPPORTED;
			if(ok){
				if(desc){ desc[2 * nr] = (uint32_t)nw; desc[2 * nr + 1] = first | n << 8; }
				if(weights) memcpy(weights + nw, w + first, n * sizeof(float));
				nr++; nw += n;
			}
		}
		if(!c0) break;
		if(c0 < prev_cmin) return BSA_E_UNSUPPORTED;
		prev_cmin = c0;
		if(cmin) cmin[a] = c0;
		if(rowbase) rowbase[a] = (uint32_t)(nr - (max_rows - c0 + 1));
	}
	// (an altn without rows ends the list: a larger one has none either, its rate is larger at every covn)
	for(uint32_t b = a + 1; b <= max_rows; b++){
		uint32_t first, n;
		for(uint32_t c = b; c <= max_rows; c++) if(snv_row(lf, b, c, &first, &n, w)) return BSA_E_UNSUPPORTED;
	}
	if(amax) *amax = a - 1;
	if(rowbase) rowbase[a] = (uint32_t)nr;
	if(nrows) *nrows = nr;
	if(nweights) *nweights = nw;
	return BSA_OK;
}
