/*
 * standin.c -- bodies for the stand-in sonLib.h / bioioC.h / pairwiseAlignment.h (test infrastructure).
 *
 * Small real bodies for what the recorded cases reach (array list, integer tuple, sorted set, a few string and file
 * helpers, allocation, logging); stubs that print their own name and abort for what they must not reach (the JSON
 * parsers and the lastz shell-out).  What these bodies could get wrong is container semantics only: the arithmetic
 * under test is all in the reference's own two files.
 */
#include "sonLib.h"
#include "bioioC.h"
#include "pairwiseAlignment.h"

#include <ctype.h>
#include <stdarg.h>

/* ---- memory, logging, abort ---- */

void *st_malloc(size_t size) {
    void *p = malloc(size > 0 ? size : 1);
    if (p == NULL) {
        fprintf(stderr, "st_malloc: out of memory\n");
        abort();
    }
    return p;
}

void *st_calloc(size_t n, size_t size) {
    void *p = calloc(n > 0 ? n : 1, size > 0 ? size : 1);
    if (p == NULL) {
        fprintf(stderr, "st_calloc: out of memory\n");
        abort();
    }
    return p;
}

void st_logDebug(const char *format, ...) {
    (void) format; /* the log level is never raised */
}

void st_errAbort(const char *format, ...) {
    va_list ap;
    va_start(ap, format);
    fprintf(stderr, "st_errAbort: ");
    vfprintf(stderr, format, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    abort();
}

void st_errnoAbort(const char *format, ...) {
    va_list ap;
    va_start(ap, format);
    fprintf(stderr, "st_errnoAbort: ");
    vfprintf(stderr, format, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    abort();
}

void stStandin_throw(const char *id, const char *format, ...) {
    va_list ap;
    va_start(ap, format);
    fprintf(stderr, "stThrowNew: %s: ", id);
    vfprintf(stderr, format, ap);
    va_end(ap);
    fprintf(stderr, "\n");
    abort();
}

double st_random(void) {
    static uint64_t state = 0x2545F4914F6CDD1DULL;
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double) (state >> 11) / 9007199254740992.0; /* [0, 1) */
}

/* ---- array list ---- */

struct _stList {
    void **items;
    int64_t length, capacity;
    void (*destructElement)(void *);
};

stList *stList_construct3(int64_t length, void (*destructElement)(void *)) {
    stList *list = st_malloc(sizeof(stList));
    list->capacity = length > 4 ? length : 4;
    list->items = st_calloc(list->capacity, sizeof(void *));
    list->length = length;
    list->destructElement = destructElement;
    return list;
}

stList *stList_construct(void) {
    return stList_construct3(0, NULL);
}

void stList_destruct(stList *list) {
    if (list->destructElement != NULL) {
        for (int64_t i = 0; i < list->length; i++) {
            if (list->items[i] != NULL) {
                list->destructElement(list->items[i]);
            }
        }
    }
    free(list->items);
    free(list);
}

int64_t stList_length(stList *list) {
    return list->length;
}

void *stList_get(stList *list, int64_t index) {
    assert(index >= 0 && index < list->length);
    return list->items[index];
}

void stList_set(stList *list, int64_t index, void *item) {
    assert(index >= 0 && index < list->length);
    list->items[index] = item;
}

void stList_append(stList *list, void *item) {
    if (list->length == list->capacity) {
        list->capacity *= 2;
        list->items = realloc(list->items, list->capacity * sizeof(void *));
        if (list->items == NULL) {
            fprintf(stderr, "stList_append: out of memory\n");
            abort();
        }
    }
    list->items[list->length++] = item;
}

void stList_appendAll(stList *list, stList *other) {
    for (int64_t i = 0; i < other->length; i++) {
        stList_append(list, other->items[i]);
    }
}

void *stList_pop(stList *list) {
    assert(list->length > 0);
    return list->items[--list->length];
}

void stList_reverse(stList *list) {
    for (int64_t i = 0, j = list->length - 1; i < j; i++, j--) {
        void *t = list->items[i];
        list->items[i] = list->items[j];
        list->items[j] = t;
    }
}

/* qsort hands the compare function pointers to the slots; the callers' functions take the items themselves */
static int (*sortCmp)(const void *, const void *);

static int sortTrampoline(const void *a, const void *b) {
    return sortCmp(*(void *const *) a, *(void *const *) b);
}

void stList_sort(stList *list, int (*cmp)(const void *a, const void *b)) {
    sortCmp = cmp;
    qsort(list->items, list->length, sizeof(void *), sortTrampoline);
}

void stList_setDestructor(stList *list, void (*destructElement)(void *)) {
    list->destructElement = destructElement;
}

/* ---- integer tuple ---- */

struct _stIntTuple {
    int64_t length;
    int64_t v[4];
};

stIntTuple *stIntTuple_construct3(int64_t a, int64_t b, int64_t c) {
    stIntTuple *t = st_malloc(sizeof(stIntTuple));
    t->length = 3;
    t->v[0] = a;
    t->v[1] = b;
    t->v[2] = c;
    t->v[3] = 0;
    return t;
}

stIntTuple *stIntTuple_construct4(int64_t a, int64_t b, int64_t c, int64_t d) {
    stIntTuple *t = stIntTuple_construct3(a, b, c);
    t->length = 4;
    t->v[3] = d;
    return t;
}

void stIntTuple_destruct(stIntTuple *tuple) {
    free(tuple);
}

int64_t stIntTuple_length(stIntTuple *tuple) {
    return tuple->length;
}

int64_t stIntTuple_get(stIntTuple *tuple, int64_t index) {
    assert(index >= 0 && index < tuple->length);
    return tuple->v[index];
}

int stIntTuple_cmpFn(stIntTuple *a, stIntTuple *b) {
    int64_t n = a->length < b->length ? a->length : b->length;
    for (int64_t i = 0; i < n; i++) {
        if (a->v[i] != b->v[i]) {
            return a->v[i] < b->v[i] ? -1 : 1;
        }
    }
    return a->length == b->length ? 0 : (a->length < b->length ? -1 : 1);
}

/* ---- sorted set: a sorted array ---- */

struct _stSortedSet {
    void **items;
    int64_t length, capacity;
    int (*cmp)(const void *, const void *);
    void (*destructElement)(void *);
};

stSortedSet *stSortedSet_construct3(int (*cmp)(const void *, const void *), void (*destructElement)(void *)) {
    stSortedSet *set = st_malloc(sizeof(stSortedSet));
    set->capacity = 8;
    set->items = st_calloc(set->capacity, sizeof(void *));
    set->length = 0;
    set->cmp = cmp;
    set->destructElement = destructElement;
    return set;
}

/* first index whose item is not below `item`; *found when that item compares equal */
static int64_t sortedSetLowerBound(stSortedSet *set, void *item, bool *found) {
    int64_t lo = 0, hi = set->length;
    while (lo < hi) {
        int64_t mid = lo + (hi - lo) / 2;
        if (set->cmp(set->items[mid], item) < 0) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    *found = lo < set->length && set->cmp(set->items[lo], item) == 0;
    return lo;
}

void stSortedSet_insert(stSortedSet *set, void *item) {
    bool found;
    int64_t at = sortedSetLowerBound(set, item, &found);
    if (found) {
        set->items[at] = item;
        return;
    }
    if (set->length == set->capacity) {
        set->capacity *= 2;
        set->items = realloc(set->items, set->capacity * sizeof(void *));
        if (set->items == NULL) {
            fprintf(stderr, "stSortedSet_insert: out of memory\n");
            abort();
        }
    }
    memmove(set->items + at + 1, set->items + at, (set->length - at) * sizeof(void *));
    set->items[at] = item;
    set->length++;
}

void *stSortedSet_search(stSortedSet *set, void *item) {
    bool found;
    int64_t at = sortedSetLowerBound(set, item, &found);
    return found ? set->items[at] : NULL;
}

void stSortedSet_destruct(stSortedSet *set) {
    if (set->destructElement != NULL) {
        for (int64_t i = 0; i < set->length; i++) {
            set->destructElement(set->items[i]);
        }
    }
    free(set->items);
    free(set);
}

/* ---- strings and files ---- */

char *stString_print(const char *format, ...) {
    va_list ap;
    va_start(ap, format);
    int n = vsnprintf(NULL, 0, format, ap);
    va_end(ap);
    char *s = st_malloc((size_t) n + 1);
    va_start(ap, format);
    vsnprintf(s, (size_t) n + 1, format, ap);
    va_end(ap);
    return s;
}

char *stString_copy(const char *s) {
    size_t n = strlen(s);
    char *t = st_malloc(n + 1);
    memcpy(t, s, n + 1);
    return t;
}

char *stString_getSubString(const char *s, int64_t start, int64_t length) {
    assert(start >= 0 && length >= 0);
    char *t = st_malloc((size_t) length + 1);
    memcpy(t, s + start, (size_t) length);
    t[length] = '\0';
    return t;
}

stList *stString_split(const char *s) {
    stList *tokens = stList_construct3(0, free);
    while (*s != '\0') {
        while (*s != '\0' && isspace((unsigned char) *s)) {
            s++;
        }
        const char *e = s;
        while (*e != '\0' && !isspace((unsigned char) *e)) {
            e++;
        }
        if (e > s) {
            stList_append(tokens, stString_getSubString(s, 0, e - s));
        }
        s = e;
    }
    return tokens;
}

char *stFile_getLineFromFile(FILE *f) {
    size_t capacity = 256, n = 0;
    char *line = st_malloc(capacity);
    int ch = fgetc(f);
    if (ch == EOF) {
        free(line);
        return NULL;
    }
    while (ch != EOF && ch != '\n') {
        if (n + 1 == capacity) {
            capacity *= 2;
            line = realloc(line, capacity);
            if (line == NULL) {
                fprintf(stderr, "stFile_getLineFromFile: out of memory\n");
                abort();
            }
        }
        line[n++] = (char) ch;
        ch = fgetc(f);
    }
    line[n] = '\0';
    return line;
}

/* ---- stubs: each names itself, then aborts ---- */

#define STUB(name)                                                        \
    do {                                                                  \
        fprintf(stderr, "stand-in stub reached: %s\n", name);             \
        abort();                                                          \
    } while (0)

int64_t st_system(const char *format, ...) {
    (void) format;
    STUB("st_system");
}

int64_t stJson_setupParser(char *buf, size_t r, jsmntok_t **tokens, char **js) {
    (void) buf, (void) r, (void) tokens, (void) js;
    STUB("stJson_setupParser");
}

char *stJson_token_tostr(char *js, jsmntok_t *t) {
    (void) js, (void) t;
    STUB("stJson_token_tostr");
}

double stJson_parseFloat(char *js, jsmntok_t *tokens, int64_t index) {
    (void) js, (void) tokens, (void) index;
    STUB("stJson_parseFloat");
}

int64_t stJson_parseInt(char *js, jsmntok_t *tokens, int64_t index) {
    (void) js, (void) tokens, (void) index;
    STUB("stJson_parseInt");
}

bool stJson_parseBool(char *js, jsmntok_t *tokens, int64_t index) {
    (void) js, (void) tokens, (void) index;
    STUB("stJson_parseBool");
}

int64_t stJson_parseFloatArray(double *out, int64_t n, char *js, jsmntok_t *tokens, int64_t index) {
    (void) out, (void) n, (void) js, (void) tokens, (void) index;
    STUB("stJson_parseFloatArray");
}

char *getTempFile(void) {
    STUB("getTempFile");
}

void fastaWrite(char *sequence, char *header, FILE *file) {
    (void) sequence, (void) header, (void) file;
    STUB("fastaWrite");
}

struct PairwiseAlignment *cigarRead(FILE *file) {
    (void) file;
    STUB("cigarRead");
}

void destructPairwiseAlignment(struct PairwiseAlignment *pA) {
    (void) pA;
    STUB("destructPairwiseAlignment");
}
