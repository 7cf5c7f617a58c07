/*
 * bioioC.h -- STAND-IN (test infrastructure; see sonLib.h beside it).  The reference reaches these two only on its
 * lastz shell-out (getBlastPairs), which no recorded case takes: they are stubs that name themselves and abort.
 */
#ifndef REF_STANDIN_BIOIOC_H_
#define REF_STANDIN_BIOIOC_H_

#include <stdio.h>

char *getTempFile(void);
void fastaWrite(char *sequence, char *header, FILE *file);

#endif
