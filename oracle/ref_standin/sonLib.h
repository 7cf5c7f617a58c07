/*
 * sonLib.h -- STAND-IN (test infrastructure).  Declarations only, written from the undefined symbols and the call sites
 * of the reference's impl/pairwiseAligner.c and impl/stateMachine.c so that those two files compile unchanged
 * (oracle/Makefile, target `ref`).  The bodies are in standin.c.  Nothing here comes from sonLib itself: the containers
 * keep sonLib's observable behaviour at those call sites (an array list, an integer tuple, a set ordered by a compare
 * function) and nothing more.
 */
#ifndef REF_STANDIN_SONLIB_H_
#define REF_STANDIN_SONLIB_H_

#include <assert.h>
#include <inttypes.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef TRUE
#define TRUE 1
#endif
#ifndef FALSE
#define FALSE 0
#endif

/* log(1): what the ragged-end state functions return */
#define LOG_ONE 0.0

/* ---- memory, logging, abort ---- */
void *st_malloc(size_t size);
void *st_calloc(size_t n, size_t size);
void st_logDebug(const char *format, ...);
void st_errAbort(const char *format, ...);
void st_errnoAbort(const char *format, ...);
int64_t st_system(const char *format, ...);
double st_random(void); /* a fixed LCG: no fixture may depend on it */

/* The reference throws at one place (an invalid diagonal); the stand-in prints the message and aborts. */
void stStandin_throw(const char *id, const char *format, ...);
#define stThrowNew(id, ...) stStandin_throw(id, __VA_ARGS__)

/* ---- array list ---- */
typedef struct _stList stList;
stList *stList_construct(void);
stList *stList_construct3(int64_t length, void (*destructElement)(void *));
void stList_destruct(stList *list);
int64_t stList_length(stList *list);
void *stList_get(stList *list, int64_t index);
void stList_set(stList *list, int64_t index, void *item);
void stList_append(stList *list, void *item);
void stList_appendAll(stList *list, stList *other);
void *stList_pop(stList *list);
void stList_reverse(stList *list);
void stList_sort(stList *list, int (*cmp)(const void *a, const void *b));
void stList_setDestructor(stList *list, void (*destructElement)(void *));

/* ---- integer tuple ---- */
typedef struct _stIntTuple stIntTuple;
stIntTuple *stIntTuple_construct3(int64_t a, int64_t b, int64_t c);
stIntTuple *stIntTuple_construct4(int64_t a, int64_t b, int64_t c, int64_t d);
void stIntTuple_destruct(stIntTuple *tuple);
int64_t stIntTuple_length(stIntTuple *tuple);
int64_t stIntTuple_get(stIntTuple *tuple, int64_t index);
int stIntTuple_cmpFn(stIntTuple *a, stIntTuple *b);

/* ---- sorted set (construct, insert, search, destruct are all the reference uses) ---- */
typedef struct _stSortedSet stSortedSet;
stSortedSet *stSortedSet_construct3(int (*cmp)(const void *, const void *), void (*destructElement)(void *));
void stSortedSet_insert(stSortedSet *set, void *item);
void *stSortedSet_search(stSortedSet *set, void *item);
void stSortedSet_destruct(stSortedSet *set);

/* ---- strings and files ---- */
char *stString_print(const char *format, ...);
char *stString_copy(const char *s);
char *stString_getSubString(const char *s, int64_t start, int64_t length);
stList *stString_split(const char *s); /* on white space; the list owns the tokens */
char *stFile_getLineFromFile(FILE *f);  /* without the newline; NULL at end of file */

/* ---- JSON: declared so the parsers compile; every one is a stub that names itself and aborts ---- */
typedef struct {
    int type, start, end, size;
} jsmntok_t;
int64_t stJson_setupParser(char *buf, size_t r, jsmntok_t **tokens, char **js);
char *stJson_token_tostr(char *js, jsmntok_t *t);
double stJson_parseFloat(char *js, jsmntok_t *tokens, int64_t index);
int64_t stJson_parseInt(char *js, jsmntok_t *tokens, int64_t index);
bool stJson_parseBool(char *js, jsmntok_t *tokens, int64_t index);
int64_t stJson_parseFloatArray(double *out, int64_t n, char *js, jsmntok_t *tokens, int64_t index);

#endif
