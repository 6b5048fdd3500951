// snv_replay.cpp -- bsa_msa_call_snvs and bsa_msa_snv_text (bsalign_amd/csrc/bsa_snv.cpp) in a stand-alone program, for a run of the host code under
// a sanitizer without Python in the process:
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude tools/snv_replay.cpp bsalign_amd/csrc/bsa_snv.cpp -o snv_replay
//     python -c "import sys; sys.path.insert(0, 'tests'); import snv_cases as SC; SC.dump_golden(0, 'set0.bin')" && ./snv_replay set0.bin
// The file holds one set of tests/golden/snv.npz: uint32 nall, nseq, mlen, nrec, text bytes; the columns, mlen x (nall + 3) bytes; nrec x 8 int64
// (mpos cpos qual covn refn altn refb altb); the SNP lines.  The program calls with skip_first_row 1, once to count and once to fill, compares
// records and text, and also runs the device model's tables (bsa_snv_model_internal) at depths 0, 40 and 1000.  Exit status 0: all equal.
#include "bsalign_msa.h"
#include "bsalign_hip.h"
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int bsa_snv_model_internal(uint32_t max_rows, double *lfv, double *lgp, double *lg1p, float *pgrid, double *ln10, uint32_t *amax, uint32_t *cmin, uint32_t *rowbase,
		uint32_t *desc, float *weights, size_t *nrows, size_t *nweights);

int main(int argc, char **argv){
	if(argc != 2){ fprintf(stderr, "usage: snv_replay <set.bin>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if(!f){ perror(argv[1]); return 2; }
	uint32_t h[5];
	if(fread(h, 4, 5, f) != 5) return 2;
	const uint32_t nall = h[0], nseq = h[1], mlen = h[2], nrec = h[3], ntext = h[4];
	std::vector<uint8_t> cols((size_t)mlen * (nall + 3));
	std::vector<int64_t> want((size_t)nrec * 8);
	std::vector<char> text(ntext);
	if(fread(cols.data(), 1, cols.size(), f) != cols.size() || fread(want.data(), 8, want.size(), f) != want.size() || fread(text.data(), 1, ntext, f) != ntext) return 2;
	fclose(f);
	const bsa_snv_params_t par = { 3, 0.5f, 5u, 1u };
	size_t n = 0; float pexp = 0; uint32_t nsites = 0;
	int rc = bsa_msa_call_snvs(cols.data(), nullptr, nall, nseq, mlen, &par, nullptr, 0, &n, &pexp, &nsites);
	if((rc != BSA_OK && rc != BSA_E_NOMEM) || n != nrec){ fprintf(stderr, "count: rc %d, %zu records, %u expected\n", rc, n, nrec); return 1; }
	std::vector<bsa_snv_t> snv(n);                                  // exactly the need: a record too many is a heap overflow the sanitizer sees
	rc = bsa_msa_call_snvs(cols.data(), nullptr, nall, nseq, mlen, &par, snv.data(), n, &n, &pexp, &nsites);
	if(rc != BSA_OK) return 1;
	for(size_t k = 0; k < n; k++){
		const int64_t got[8] = { snv[k].mpos, snv[k].cpos, snv[k].qual, snv[k].covn, snv[k].refn, snv[k].altn, snv[k].refb, snv[k].altb };
		if(memcmp(got, &want[k * 8], sizeof(got)) != 0){ fprintf(stderr, "record %zu differs\n", k); return 1; }
	}
	std::vector<uint8_t> cns, qlt;
	for(uint32_t i = 0; i < mlen; i++){
		const uint8_t *c = &cols[(size_t)i * (nall + 3)];
		if(c[nall] < 4){ cns.push_back(c[nall]); qlt.push_back(c[nall + 1]); }
	}
	size_t need = 0;
	rc = bsa_msa_snv_text(cols.data(), nullptr, nall, nseq, mlen, cns.data(), qlt.data(), (uint32_t)cns.size(), snv.data(), n, "BSALIGN", nullptr, 0, &need);
	if((rc != BSA_OK && rc != BSA_E_NOMEM) || need != ntext){ fprintf(stderr, "text: rc %d, %zu bytes, %u expected\n", rc, need, ntext); return 1; }
	std::vector<char> out(need);
	rc = bsa_msa_snv_text(cols.data(), nullptr, nall, nseq, mlen, cns.data(), qlt.data(), (uint32_t)cns.size(), snv.data(), n, "BSALIGN", out.data(), need, &need);
	if(need && (rc != BSA_OK || memcmp(out.data(), text.data(), need) != 0)){ fprintf(stderr, "text differs\n"); return 1; }
	for(uint32_t max_rows : { 0u, 40u, 1000u }){
		size_t nrows = 0, nw = 0; uint32_t amax = 0; double ln10 = 0;
		if(bsa_snv_model_internal(max_rows, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nrows, &nw) != BSA_OK) return 1;
		std::vector<double> lf(1001), lgp(101), lg1p(101);
		std::vector<float> pg(101), w(nw);
		std::vector<uint32_t> cmin(max_rows + 2), rb(max_rows + 2), desc(2 * nrows);
		if(bsa_snv_model_internal(max_rows, lf.data(), lgp.data(), lg1p.data(), pg.data(), &ln10, &amax, cmin.data(), rb.data(), desc.data(), w.data(), &nrows, &nw) != BSA_OK) return 1;
		printf("model %u: altn up to %u, %zu rows, %zu weights\n", max_rows, amax, nrows, nw);
	}
	printf("%zu records, rate %.4f, %u sites, %zu bytes of text: equal\n", n, pexp, nsites, need);
	return 0;
}
