/* A C99 caller of predict_X_old_collective_explicit / _implicit (include/cmfrec_hip.h): a 5 x 7 model with k_user, k_item and
 * k_main non-zero, whose entries are small multiples of 1/8 so that the test can restate them exactly; ten pairs, two of them
 * out of range.  Prints one line per call: the return code, then the predictions with 17 significant digits. */
#include <stdio.h>
#include <stddef.h>
#include <stdbool.h>
#include "cmfrec_hip.h"

#define M 5
#define N 7
#define K 3
#define K_USER 2
#define K_ITEM 1
#define K_MAIN 2
#define NP 10

int main(void)
{
    static real_t A[M * (K_USER + K + K_MAIN)], B[N * (K_ITEM + K + K_MAIN)], biasA[M], biasB[N];
    int_t row[NP] = {0, 4, 2, 2, 1, 3, 5, 0, 4, 3}, col[NP] = {0, 6, 3, 3, 5, 1, 2, 7, 0, 4};
    real_t out[NP];
    const int lda = K_USER + K + K_MAIN, ldb = K_ITEM + K + K_MAIN;
    int i, j, rc;
    for (i = 0; i < M; i++) {
        for (j = 0; j < lda; j++) A[i * lda + j] = (real_t)(((i * 7 + j * 3) % 11) - 5) / 8;
        biasA[i] = (real_t)(i - 2) / 4;
    }
    for (i = 0; i < N; i++) {
        for (j = 0; j < ldb; j++) B[i * ldb + j] = (real_t)(((i * 5 + j * 2) % 13) - 6) / 8;
        biasB[i] = (real_t)(3 - i) / 16;
    }
    rc = predict_X_old_collective_explicit(row, col, out, (size_t)NP, A, biasA, B, biasB, (real_t)1.5, K, K_USER, K_ITEM, K_MAIN, M, N, 1);
    printf("%d", rc);
    for (i = 0; i < NP; i++) printf(" %.17g", (double)out[i]);
    printf("\n");
    rc = predict_X_old_collective_implicit(row, col, out, (size_t)NP, A, B, K, K_USER, K_ITEM, K_MAIN, M, N, 1);
    printf("%d", rc);
    for (i = 0; i < NP; i++) printf(" %.17g", (double)out[i]);
    printf("\n");
    return 0;
}
